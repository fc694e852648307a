// flac.hip — FLAC decoding on the GPU for device-side ingest (load_audio(..., decode_on_device=True)): the file's
//   bytes go up as they are and come out as interleaved int32 PCM, which wh_resample takes as it takes a host decoder's.  FLAC frames
//   are independent (own header, predictor, Rice parameters, CRC-16), so one lane decodes one frame; what a frame is, is found
//   without walking the stream:
//     scan    every byte offset behind the metadata is tested as a frame start (flac_core.h: flac_candidate — sync code, reserved
//             bits, codes consistent with STREAMINFO, coded number, CRC-8).  Survivors are compacted in offset order: a count per
//             tile of 1024 offsets, one prefix sum, a second pass that writes — no atomic append, so the same bytes give the same
//             list.  Payload bytes pass the test by chance about once in 2^24.
//     decode  one lane per candidate runs flac_frame_n (flac_core.h, the code wh_flac_decode runs, with int32 storage) and writes
//             [frame][channel] int32 at the candidate's provisional position: the prefix sum of the candidates' block sizes.  It
//             records the frame's end offset and its status (the CRC-16 over [start, end) among the checks).  A false candidate
//             is a bounded parse of garbage that stores inside its own block of the staging buffer and nowhere else.
//     chain   start / end / block size / status of every candidate are downloaded and walked on the host (flac_core.h:
//             flac_chain): sorted candidates, a monotone chain, one linear pass.
//     compact if every candidate was chained — the normal case — the staging buffer is the output.  Otherwise the chained frames
//             are copied to their final places in a second buffer and back.
//   The kernels here; the sequence and the wait are wh_flac_decode_device (api.cpp).  The arithmetic is integer: the PCM equals
//   wh_flac_decode's bit for bit.  Not verified here: the STREAMINFO MD5 (serial over all PCM).
#include "common.h"
#include "kernels.h"

#include "flac_core.h"
#define FLAC_T int32_t
#define FLAC_SUFFIX _n
#include "flac_core.h"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER = 4;                          // offsets per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_PER;   // offsets per workgroup
constexpr int PREFIX_THREADS = 1024;
constexpr int DECODE_THREADS = 64;                   // one wave per workgroup: the frames spread over the CUs

// exclusive prefix of v over the workgroup (THREADS a power of two); *total = the workgroup's sum
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive(T v, T* lds, T* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    const T add = t >= d ? lds[t - d] : (T)0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const T incl = lds[t];
  *total = lds[THREADS - 1];
  __syncthreads();
  return incl - v;
}

// WRITE == false: tile_count[tile] = candidates among the tile's offsets.  WRITE == true: the candidates themselves, at
// tile_base[tile] + their rank inside the tile (entries at or beyond max_cand are dropped; hdr[1] keeps the full count)
template <bool WRITE>
__global__ __launch_bounds__(SCAN_THREADS) void flac_scan_kernel(const uint8_t* __restrict__ file, size_t size, size_t first, int ch,
                                                                 int bps, int max_block, int* __restrict__ tile_count,
                                                                 const int* __restrict__ tile_base, int64_t* __restrict__ start,
                                                                 int* __restrict__ bs, int max_cand) {
  __shared__ int lds[SCAN_THREADS];
  const size_t p0 = first + (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
  int found[SCAN_PER];
  int n = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PER; ++k) {
    found[k] = flac_candidate(file, size, p0 + k, ch, bps, max_block);      // 0 past the end of the file
    n += found[k] != 0;
  }
  int total;
  int rank = block_exclusive<SCAN_THREADS>(n, lds, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
    return;
  }
  rank += tile_base[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_PER; ++k) {
    if (!found[k]) continue;
    if (rank < max_cand) { start[rank] = (int64_t)(p0 + k); bs[rank] = found[k]; }
    ++rank;
  }
}

// out[i] = in[0] + ... + in[i - 1] for i < n, *sum_out = the sum (clamped to int32); one workgroup, n = n_value or min(*n_dev, n_limit)
template <typename Out>
__global__ __launch_bounds__(PREFIX_THREADS) void flac_prefix_kernel(const int* __restrict__ in, Out* __restrict__ out, int64_t n_value,
                                                                     const int* __restrict__ n_dev, int n_limit, int* sum_out,
                                                                     int* n_clipped_out) {
  __shared__ Out lds[PREFIX_THREADS];
  int64_t n = n_value;
  if (n_dev) { n = *n_dev; if (n > n_limit) n = n_limit; }
  Out carry = 0;
  for (int64_t base = 0; base < n; base += PREFIX_THREADS) {
    const int64_t i = base + threadIdx.x;
    const Out v = i < n ? (Out)in[i] : (Out)0;
    Out total;
    const Out ex = block_exclusive<PREFIX_THREADS>(v, lds, &total);
    if (i < n) out[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (sum_out) *sum_out = carry > (Out)0x7fffffff ? 0x7fffffff : (int)carry;
    if (n_clipped_out) *n_clipped_out = (int)n;
  }
}

// hdr[0] = candidates listed (<= max_cand), hdr[1] = candidates found; tail = the file's last min(size, FLAC_TAIL) bytes
__global__ void flac_decode_kernel(const uint8_t* __restrict__ file, size_t size, int ch, int bps, const int* __restrict__ hdr,
                                   const int64_t* __restrict__ start, const int* __restrict__ bs, const int64_t* __restrict__ prov,
                                   int64_t* __restrict__ end, int* __restrict__ rc, int32_t* __restrict__ pcm, int64_t staging_frames,
                                   uint8_t* __restrict__ tail) {
  if (blockIdx.x == 0) {
    const size_t tail_len = size < (size_t)FLAC_TAIL ? size : (size_t)FLAC_TAIL;
    for (size_t i = threadIdx.x; i < tail_len; i += blockDim.x) tail[i] = file[size - tail_len + i];
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= hdr[0]) return;
  const size_t pos = (size_t)start[j];
  size_t e = pos;
  int status;
  if (prov[j] < 0 || prov[j] + bs[j] > staging_frames) {
    status = FLAC_E_MEM;                               // no room in the staging buffer: not decoded
  } else {
    flac_hdr h;
    int range = 0;
    status = flac_frame_n(file, size, pos, ch, bps, bs[j], pcm + prov[j] * ch, 1, (size_t)ch, &h, &e, &range);
    if (status == FLAC_OK && range) status = FLAC_E_RANGE;
  }
  end[j] = (int64_t)e;
  rc[j] = status;
}

// move k: len[k] int32 from src + from[k] to dst + to[k]; one workgroup per move
__global__ __launch_bounds__(256) void flac_move_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                        const int64_t* __restrict__ from, const int64_t* __restrict__ to,
                                                        const int* __restrict__ len) {
  const int k = blockIdx.x;
  const int32_t* s = src + from[k];
  int32_t* d = dst + to[k];
  for (int i = threadIdx.x; i < len[k]; i += 256) d[i] = s[i];
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

namespace whk {

FlacScratch flac_scratch(void* base, size_t size, int channels, int64_t staging_frames, int max_cand) {
  FlacScratch s;
  uint8_t* p = (uint8_t*)base;
  size_t at = 0;
  const size_t m = (size_t)max_cand;
  auto take = [&](size_t bytes) { uint8_t* q = p + at; at += up256(bytes); return q; };
  s.hdr = (int*)take(64);                               // records, downloaded in one copy: hdr .. rc
  s.tail = take(FLAC_TAIL);
  s.start = (int64_t*)take(m * 8);
  s.end = (int64_t*)take(m * 8);
  s.bs = (int*)take(m * 4);
  s.rc = (int*)take(m * 4);
  s.record_bytes = at;
  s.prov = (int64_t*)take(m * 8);
  const size_t tiles = size / SCAN_TILE + 1;
  s.tile_count = (int*)take(tiles * 4);
  s.tile_base = (int*)take(tiles * 4);
  s.mv_from = (int64_t*)take(m * 8);
  s.mv_to = (int64_t*)take(m * 8);
  s.mv_len = (int*)take(m * 4);
  s.temp = (int32_t*)take((size_t)staging_frames * channels * 4);
  s.total_bytes = at;
  return s;
}

hipError_t launch_flac_scan(const uint8_t* file, size_t size, size_t first, int ch, int bps, int max_block, const FlacScratch& s,
                            int max_cand, hipStream_t stream) {
  const size_t span = size - first;                   // first < size (caller)
  const size_t tiles = (span + SCAN_TILE - 1) / SCAN_TILE;
  if (tiles > 0x7fffffffULL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles), block(SCAN_THREADS);
  hipLaunchKernelGGL(flac_scan_kernel<false>, grid, block, 0, stream, file, size, first, ch, bps, max_block, s.tile_count,
                     (const int*)nullptr, (int64_t*)nullptr, (int*)nullptr, max_cand);
  hipLaunchKernelGGL(flac_prefix_kernel<int>, dim3(1), dim3(PREFIX_THREADS), 0, stream, (const int*)s.tile_count, s.tile_base,
                     (int64_t)tiles, (const int*)nullptr, 0, s.hdr + 1, (int*)nullptr);
  hipLaunchKernelGGL(flac_scan_kernel<true>, grid, block, 0, stream, file, size, first, ch, bps, max_block, (int*)nullptr,
                     (const int*)s.tile_base, s.start, s.bs, max_cand);
  // provisional positions: the prefix sum of the listed candidates' block sizes; hdr[0] = how many are listed
  hipLaunchKernelGGL(flac_prefix_kernel<int64_t>, dim3(1), dim3(PREFIX_THREADS), 0, stream, (const int*)s.bs, s.prov, (int64_t)0,
                     (const int*)(s.hdr + 1), max_cand, (int*)nullptr, s.hdr);
  return hipGetLastError();
}

hipError_t launch_flac_decode(const uint8_t* file, size_t size, int ch, int bps, const FlacScratch& s, int max_cand, int32_t* pcm,
                              int64_t staging_frames, hipStream_t stream) {
  const unsigned blocks = (unsigned)((max_cand + DECODE_THREADS - 1) / DECODE_THREADS);
  hipLaunchKernelGGL(flac_decode_kernel, dim3(blocks), dim3(DECODE_THREADS), 0, stream, file, size, ch, bps, (const int*)s.hdr,
                     (const int64_t*)s.start, (const int*)s.bs, (const int64_t*)s.prov, s.end, s.rc, pcm, staging_frames, s.tail);
  return hipGetLastError();
}

hipError_t launch_flac_move(const int32_t* src, int32_t* dst, const FlacScratch& s, int n_moves, hipStream_t stream) {
  if (n_moves <= 0) return hipSuccess;
  hipLaunchKernelGGL(flac_move_kernel, dim3((unsigned)n_moves), dim3(256), 0, stream, src, dst, (const int64_t*)s.mv_from,
                     (const int64_t*)s.mv_to, (const int*)s.mv_len);
  return hipGetLastError();
}

}  // namespace whk
