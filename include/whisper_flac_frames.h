/*
 * whisper_flac_frames.h — the frame-parallel FLAC decode, run serially on the host (libwhisper_audio.so,
 * whisper_amd/csrc/flac_decode.c).  It is the twin of the GPU route wh_flac_decode_device (whisper_hip.h,
 * csrc/flac.hip), built from the same per-frame core (csrc/flac_core.h), so that the algorithm — false sync
 * candidates, the chain, the compaction — can be tested and run under sanitizers without a GPU.
 */
#ifndef WHISPER_FLAC_FRAMES_H
#define WHISPER_FLAC_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scan every byte offset behind the metadata for a frame header that holds, decode every candidate on its own, chain the
 * candidates that continue each other from the first frame on, close the gaps the others left.  Results as
 * wh_flac_decode (release *samples with wh_flac_free), except that the STREAMINFO MD5 signature is not verified: every
 * frame's CRC-8 and CRC-16, the unbroken chain and the sample count are.
 * Returns 0, a metadata error of wh_flac_decode, -5 for a stream the route does not take (more than 24 bits per sample,
 * no sample count in STREAMINFO) or -10 when the stream fails its checks.
 * stats (optional, int32[4]): candidates, chained frames, 1 if the staging buffer was compacted, 0.
 * cand_start / cand_bs / cand_end / cand_rc (optional, cand_cap entries each): every candidate's start offset, block size,
 * end offset (behind its CRC-16; its start offset when the body could not be parsed) and decode status. */
int wh_flac_decode_frames(const uint8_t *data, size_t size, int32_t **samples, int64_t *n_frames, int *channels,
                          int *sample_rate, int *bits_per_sample, int32_t *stats, int64_t *cand_start, int32_t *cand_bs,
                          int64_t *cand_end, int32_t *cand_rc, int cand_cap);

/* Samples per channel of staging the frame-parallel routes want for a stream of `total` samples per channel. */
uint64_t wh_flac_staging_frames(uint64_t total);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_FLAC_FRAMES_H */
