/*
 * flac_decode.c — a small native FLAC decoder for whisper_amd.audio.load_audio.
 *
 * The reference decodes every input through the ffmpeg CLI (whisper/audio.py:25-62).  When ffmpeg is not
 * installed, whisper_amd reads RIFF/WAVE natively in Python and FLAC through this file (built by gcc into
 * whisper_amd/libwhisper_audio.so — host code, no HIP).  It implements the FLAC stream format as published
 * (xiph.org FLAC format / RFC 9639): STREAMINFO, frame headers with CRC-8 and CRC-16, CONSTANT / VERBATIM /
 * FIXED / LPC subframes, partitioned Rice residuals (4- and 5-bit parameters, escape partitions), wasted bits,
 * all stereo decorrelation modes, 4..32 bits per sample, and checks the decoded audio against the MD5
 * signature stored in STREAMINFO.  Output: interleaved int32 samples.
 *
 *   int  wh_flac_decode(const uint8_t* data, size_t size, int32_t** samples, int64_t* n_frames,
 *                       int* channels, int* sample_rate, int* bits_per_sample);   // 0 = ok, < 0 = error code
 *   void wh_flac_free(int32_t* samples);
 *   const char* wh_flac_error(int code);
 *
 * The per-frame logic (bit reader, CRCs, frame header, subframes, decorrelation) lives in flac_core.h, which csrc/flac.hip
 * compiles a second time as device code.  wh_flac_decode_frames (include/whisper_flac_frames.h) is the serial twin of that
 * GPU route: the same scan -> per-candidate decode -> chain -> compact algorithm, testable without a GPU.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "flac_core.h"
#define FLAC_T int64_t
#define FLAC_SUFFIX _w
#include "flac_core.h"
#define FLAC_T int32_t
#define FLAC_SUFFIX _n
#include "flac_core.h"
#include "../../include/whisper_flac_frames.h"

const char* wh_flac_error(int code) {
  switch (code) {
    case FLAC_OK: return "ok";
    case FLAC_E_MAGIC: return "not a FLAC stream (missing fLaC marker)";
    case FLAC_E_TRUNC: return "truncated FLAC stream";
    case FLAC_E_HEADER: return "invalid FLAC frame or metadata header";
    case FLAC_E_CRC: return "FLAC frame CRC mismatch";
    case FLAC_E_UNSUP: return "unsupported FLAC feature";
    case FLAC_E_MD5: return "decoded audio does not match the MD5 signature in STREAMINFO";
    case FLAC_E_MEM: return "out of memory";
    case FLAC_E_SYNC: return "lost FLAC frame sync";
    default: return "unknown FLAC error";
  }
}

/* ---------------------------------------------------------------- MD5 (RFC 1321) */
typedef struct { uint32_t h[4]; uint64_t len; uint8_t buf[64]; size_t fill; } MD5;
static const uint32_t md5_k[64] = {
  0xd76aa478,0xe8c7b756,0x242070db,0xc1bdceee,0xf57c0faf,0x4787c62a,0xa8304613,0xfd469501,0x698098d8,0x8b44f7af,0xffff5bb1,0x895cd7be,
  0x6b901122,0xfd987193,0xa679438e,0x49b40821,0xf61e2562,0xc040b340,0x265e5a51,0xe9b6c7aa,0xd62f105d,0x02441453,0xd8a1e681,0xe7d3fbc8,
  0x21e1cde6,0xc33707d6,0xf4d50d87,0x455a14ed,0xa9e3e905,0xfcefa3f8,0x676f02d9,0x8d2a4c8a,0xfffa3942,0x8771f681,0x6d9d6122,0xfde5380c,
  0xa4beea44,0x4bdecfa9,0xf6bb4b60,0xbebfbc70,0x289b7ec6,0xeaa127fa,0xd4ef3085,0x04881d05,0xd9d4d039,0xe6db99e5,0x1fa27cf8,0xc4ac5665,
  0xf4292244,0x432aff97,0xab9423a7,0xfc93a039,0x655b59c3,0x8f0ccc92,0xffeff47d,0x85845dd1,0x6fa87e4f,0xfe2ce6e0,0xa3014314,0x4e0811a1,
  0xf7537e82,0xbd3af235,0x2ad7d2bb,0xeb86d391};
static const uint8_t md5_r[64] = {7,12,17,22,7,12,17,22,7,12,17,22,7,12,17,22,5,9,14,20,5,9,14,20,5,9,14,20,5,9,14,20,
                                  4,11,16,23,4,11,16,23,4,11,16,23,4,11,16,23,6,10,15,21,6,10,15,21,6,10,15,21,6,10,15,21};
static void md5_block(MD5* m, const uint8_t* p) {
  uint32_t w[16], a = m->h[0], b = m->h[1], c = m->h[2], d = m->h[3];
  for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4*i] | (uint32_t)p[4*i+1] << 8 | (uint32_t)p[4*i+2] << 16 | (uint32_t)p[4*i+3] << 24;
  for (int i = 0; i < 64; ++i) {
    uint32_t f; int g;
    if (i < 16) { f = (b & c) | (~b & d); g = i; }
    else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
    else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
    else { f = c ^ (b | ~d); g = (7 * i) & 15; }
    uint32_t t = a + f + md5_k[i] + w[g];
    a = d; d = c; c = b; b = b + ((t << md5_r[i]) | (t >> (32 - md5_r[i])));
  }
  m->h[0] += a; m->h[1] += b; m->h[2] += c; m->h[3] += d;
}
static void md5_init(MD5* m) { m->h[0] = 0x67452301; m->h[1] = 0xefcdab89; m->h[2] = 0x98badcfe; m->h[3] = 0x10325476; m->len = 0; m->fill = 0; }
static void md5_update(MD5* m, const uint8_t* p, size_t n) {
  m->len += n;
  while (n) {
    size_t k = 64 - m->fill; if (k > n) k = n;
    memcpy(m->buf + m->fill, p, k); m->fill += k; p += k; n -= k;
    if (m->fill == 64) { md5_block(m, m->buf); m->fill = 0; }
  }
}
static void md5_final(MD5* m, uint8_t out[16]) {
  uint64_t bits = m->len * 8;
  uint8_t pad = 0x80; md5_update(m, &pad, 1);
  uint8_t z = 0; while (m->fill != 56) md5_update(m, &z, 1);
  uint8_t l[8]; for (int i = 0; i < 8; ++i) l[i] = (uint8_t)(bits >> (8 * i));
  md5_update(m, l, 8);
  for (int i = 0; i < 4; ++i) for (int k = 0; k < 4; ++k) out[4*i+k] = (uint8_t)(m->h[i] >> (8 * k));
}

/* ---------------------------------------------------------------- metadata */
typedef struct { int sr, ch, bps, max_block; uint64_t total; uint8_t md5[16]; size_t first; } flac_info;

static int parse_metadata(const uint8_t* data, size_t size, flac_info* fi) {
  size_t pos = 0;
  if (size >= 10 && !memcmp(data, "ID3", 3)) {        /* skip an ID3v2 tag */
    size_t tag = ((size_t)(data[6] & 127) << 21) | ((size_t)(data[7] & 127) << 14) | ((size_t)(data[8] & 127) << 7) | (data[9] & 127);
    pos = 10 + tag;
  }
  if (pos + 4 > size || memcmp(data + pos, "fLaC", 4)) return FLAC_E_MAGIC;
  pos += 4;
  int have_info = 0;
  memset(fi, 0, sizeof *fi);
  for (;;) {
    if (pos + 4 > size) return FLAC_E_TRUNC;
    int last = data[pos] >> 7, type = data[pos] & 127;
    size_t len = ((size_t)data[pos+1] << 16) | ((size_t)data[pos+2] << 8) | data[pos+3];
    pos += 4;
    if (pos + len > size) return FLAC_E_TRUNC;
    if (type == 0) {
      if (len < 34) return FLAC_E_HEADER;
      const uint8_t* q = data + pos;
      fi->max_block = (q[2] << 8) | q[3];
      fi->sr = (q[10] << 12) | (q[11] << 4) | (q[12] >> 4);
      fi->ch = ((q[12] >> 1) & 7) + 1;
      fi->bps = (((q[12] & 1) << 4) | (q[13] >> 4)) + 1;
      fi->total = ((uint64_t)(q[13] & 15) << 32) | ((uint64_t)q[14] << 24) | ((uint64_t)q[15] << 16) | ((uint64_t)q[16] << 8) | q[17];
      memcpy(fi->md5, q + 18, 16);
      have_info = 1;
    }
    pos += len;
    if (last) break;
  }
  if (!have_info || fi->sr == 0 || fi->max_block < 16 || fi->bps < 4 || fi->bps > 32) return FLAC_E_HEADER;
  fi->first = pos;
  return FLAC_OK;
}

/* ---------------------------------------------------------------- stream */
int wh_flac_decode(const uint8_t* data, size_t size, int32_t** samples_out, int64_t* n_frames_out, int* channels_out,
                   int* sample_rate_out, int* bps_out) {
  if (!data || !samples_out || !n_frames_out || !channels_out || !sample_rate_out || !bps_out) return FLAC_E_HEADER;
  *samples_out = NULL;
  flac_info fi;
  int rc = parse_metadata(data, size, &fi);
  if (rc) return rc;
  const int ch = fi.ch, bps = fi.bps;
  const uint64_t total = fi.total;
  size_t pos = fi.first;

  /* STREAMINFO's sample count sizes the output only as far as the file could possibly hold that much: a frame of
     constant subframes packs 65535 samples per channel into ~16 bytes, nothing packs more; the buffer grows anyway */
  size_t cap = (size_t)1 << 20;
  if (total && total / 4096 <= (uint64_t)size) cap = (size_t)total;
  int32_t* out = (int32_t*)malloc(cap * ch * sizeof(int32_t));
  int64_t* work = (int64_t*)malloc((size_t)65536 * 8 * sizeof(int64_t));
  if (!out || !work) { free(out); free(work); return FLAC_E_MEM; }
  size_t done = 0;

  while (pos + 2 <= size) {
    if (!flac_is_sync(data, size, pos)) {
      /* trailing bytes (e.g. an ID3v1 tag) end the stream; garbage in the middle is an error */
      if (total && done >= total) break;
      if (size - pos <= FLAC_TAIL) break;
      rc = FLAC_E_SYNC; break;
    }
    flac_hdr h; size_t end; int range = 0;
    rc = flac_frame_w(data, size, pos, ch, bps, FLAC_MAX_BLOCK, work, 65536, 1, &h, &end, &range);
    if (rc) break;
    pos = end;
    const int blocksize = h.blocksize;

    if (done + (size_t)blocksize > cap) {
      size_t ncap = cap * 2 > done + blocksize ? cap * 2 : done + blocksize;
      int32_t* n = (int32_t*)realloc(out, ncap * ch * sizeof(int32_t));
      if (!n) { rc = FLAC_E_MEM; break; }
      out = n; cap = ncap;
    }
    for (int c = 0; c < ch; ++c) {
      const int64_t* w = work + (size_t)c * 65536;
      for (int i = 0; i < blocksize; ++i) out[(done + i) * ch + c] = (int32_t)w[i];
    }
    done += blocksize;
  }
  free(work);
  if (!rc && total && done < total) rc = FLAC_E_TRUNC;
  if (!rc) {
    if (total && done > total) done = total;
    int nonzero = 0;
    for (int i = 0; i < 16; ++i) nonzero |= fi.md5[i];
    if (nonzero) {                                                    /* an all-zero signature means "not computed" */
      MD5 m; md5_init(&m);
      const int nb = (bps + 7) / 8;
      uint8_t buf[4096]; size_t fill = 0;
      for (size_t i = 0; i < done * (size_t)ch; ++i) {
        uint32_t v = (uint32_t)out[i];
        for (int k = 0; k < nb; ++k) buf[fill++] = (uint8_t)(v >> (8 * k));
        if (fill + 4 > sizeof buf) { md5_update(&m, buf, fill); fill = 0; }
      }
      md5_update(&m, buf, fill);
      uint8_t got[16]; md5_final(&m, got);
      if (memcmp(got, fi.md5, 16)) rc = FLAC_E_MD5;
    }
  }
  if (rc) { free(out); return rc; }
  *samples_out = out; *n_frames_out = (int64_t)done; *channels_out = ch; *sample_rate_out = fi.sr; *bps_out = bps;
  return FLAC_OK;
}

void wh_flac_free(int32_t* samples) { free(samples); }

/* staging capacity (samples per channel) of the frame-parallel routes for a stream of `total` samples per channel: the
 * stream itself and room for false candidates, each of which claims at most 65535 */
uint64_t wh_flac_staging_frames(uint64_t total) { return total + total / 8 + 2 * 65536; }

/* ---------------------------------------------------------------- the frame-parallel algorithm, run serially
 * What csrc/flac.hip does on the GPU, stage by stage, from the same core: scan every byte offset for a frame header that
 * holds, decode every candidate on its own into a staging buffer at the prefix sum of the candidates' block sizes, chain
 * the candidates that belong to the stream, close the gaps the others left.  The STREAMINFO MD5 is not verified (it is
 * serial over all PCM); every frame's CRC-8 and CRC-16, the unbroken chain and the sample count are.
 * FLAC_E_UNSUP: a stream this route does not take (more than 24 bits per sample, no sample count in STREAMINFO);
 * FLAC_E_REJECT: the stream fails its checks; metadata errors as wh_flac_decode reports them.
 * stats (optional, int32[4]): candidates, chained frames, 1 if the staging buffer had to be compacted, 0.
 * cand_* (optional, cand_cap entries each): the candidates' start offsets, block sizes, end offsets, decode statuses. */
int wh_flac_decode_frames(const uint8_t* data, size_t size, int32_t** samples_out, int64_t* n_frames_out, int* channels_out,
                          int* sample_rate_out, int* bps_out, int32_t* stats, int64_t* cand_start, int32_t* cand_bs,
                          int64_t* cand_end, int32_t* cand_rc, int cand_cap) {
  if (!data || !samples_out || !n_frames_out || !channels_out || !sample_rate_out || !bps_out) return FLAC_E_HEADER;
  *samples_out = NULL;
  if (stats) memset(stats, 0, 4 * sizeof(int32_t));
  flac_info fi;
  int rc = parse_metadata(data, size, &fi);
  if (rc) return rc;
  if (fi.bps > 24 || fi.total == 0) return FLAC_E_UNSUP;
  const int ch = fi.ch;
  const uint64_t cap = wh_flac_staging_frames(fi.total);

  /* scan: candidates in offset order */
  size_t n_cand = 0, room = 1024;
  int64_t* start = (int64_t*)malloc(room * sizeof(int64_t));
  int32_t* bs = (int32_t*)malloc(room * sizeof(int32_t));
  if (!start || !bs) { free(start); free(bs); return FLAC_E_MEM; }
  for (size_t pos = fi.first; pos + 2 <= size; ++pos) {
    if (data[pos] != 0xFF) continue;
    const int b = flac_candidate(data, size, pos, ch, fi.bps, fi.max_block);
    if (!b) continue;
    if (n_cand == room) {
      room *= 2;
      int64_t* ns = (int64_t*)realloc(start, room * sizeof(int64_t));
      if (ns) start = ns;
      int32_t* nb = (int32_t*)realloc(bs, room * sizeof(int32_t));
      if (nb) bs = nb;
      if (!ns || !nb) { free(start); free(bs); return FLAC_E_MEM; }
    }
    start[n_cand] = (int64_t)pos; bs[n_cand] = b; ++n_cand;
  }
  if (n_cand > 0x7fffffff) { free(start); free(bs); return FLAC_E_REJECT; }

  /* provisional positions; candidates that do not fit the staging buffer are not decoded */
  int64_t* end = (int64_t*)malloc((n_cand + 1) * sizeof(int64_t));
  int64_t* prov = (int64_t*)malloc((n_cand + 1) * sizeof(int64_t));
  int32_t* crc = (int32_t*)malloc((n_cand + 1) * sizeof(int32_t));
  int32_t* acc = (int32_t*)malloc((n_cand + 1) * sizeof(int32_t));
  uint64_t staged = 0;
  for (size_t j = 0; j < n_cand && prov; ++j) { prov[j] = (int64_t)staged; staged += (uint64_t)bs[j]; }
  if (staged > cap) staged = cap;
  int32_t* out = (int32_t*)malloc((size_t)(staged ? staged : 1) * ch * sizeof(int32_t));
  if (!end || !prov || !crc || !acc || !out) rc = FLAC_E_MEM;

  /* decode: every candidate on its own */
  for (size_t j = 0; j < n_cand && !rc; ++j) {
    flac_hdr h; size_t e = (size_t)start[j]; int range = 0;
    if ((uint64_t)prov[j] + (uint64_t)bs[j] > cap) crc[j] = FLAC_E_MEM;
    else {
      crc[j] = flac_frame_n(data, size, (size_t)start[j], ch, fi.bps, bs[j], out + (size_t)prov[j] * ch, 1, (size_t)ch, &h, &e, &range);
      if (crc[j] == FLAC_OK && range) crc[j] = FLAC_E_RANGE;
    }
    end[j] = (int64_t)e;
  }
  if (!rc) {
    const size_t nc = n_cand < (size_t)(cand_cap > 0 ? cand_cap : 0) ? n_cand : (size_t)(cand_cap > 0 ? cand_cap : 0);
    if (cand_start) memcpy(cand_start, start, nc * sizeof(int64_t));
    if (cand_bs) memcpy(cand_bs, bs, nc * sizeof(int32_t));
    if (cand_end) memcpy(cand_end, end, nc * sizeof(int64_t));
    if (cand_rc) memcpy(cand_rc, crc, nc * sizeof(int32_t));
    if (stats) stats[0] = (int32_t)n_cand;
  }

  /* chain, then compact */
  int n_acc = 0; int64_t done = 0;
  if (!rc) {
    const size_t tail_len = size < FLAC_TAIL ? size : FLAC_TAIL;
    rc = flac_chain(start, end, bs, crc, (int)n_cand, fi.first, size, data + size - tail_len, fi.total, acc, &n_acc, &done);
  }
  if (!rc) {
    if ((size_t)n_acc != n_cand) {
      int64_t at = 0;
      for (int k = 0; k < n_acc; ++k) {
        const int j = acc[k];
        if (prov[j] != at) memmove(out + (size_t)at * ch, out + (size_t)prov[j] * ch, (size_t)bs[j] * ch * sizeof(int32_t));
        at += bs[j];
      }
      if (stats) stats[2] = 1;
    }
    if (stats) stats[1] = n_acc;
    if ((uint64_t)done > fi.total) done = (int64_t)fi.total;
  }
  free(start); free(bs); free(end); free(prov); free(crc); free(acc);
  if (rc) { free(out); return rc; }
  *samples_out = out; *n_frames_out = done; *channels_out = ch; *sample_rate_out = fi.sr; *bps_out = fi.bps;
  return FLAC_OK;
}
