// chunk.hip — where to cut one long recording (transcribe_chunked; DESIGN.md §5b "Cutting a file at pauses").
//   The input is the whole-file log-mel spectrogram as log_mel_spectrogram leaves it on the device: fp32
//   M[n_mels][frame_stride], M = (x + 4) / 4 with x = max(log10(mel power), global max - 8).
//   level : L[f] = log10( (1 / n_mels) * sum_m 10^(4 M[m][f] - 4) ), 0 <= f < content   (log10 of the mean mel power)
//   cost  : C[f] = max L[g] over max(0, f - W) <= g <= min(content - 1, f + W)          (a cut needs a quiet +-W neighbourhood)
//   walk  : a = 0; while content - a > max_frames: c = the f in [a + min_frames, a + max_frames] with the smallest C,
//           the LARGEST such f among equal minima; emit c; a = c.
//   C is a sliding max of L and the walk only compares values of C: given L, cost and cuts are exact.  The launches are
//   stream-ordered; nothing here waits on the host and nothing needs an atomic.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LEVEL_THREADS = 256;
constexpr int COST_TILE = 256;
constexpr int COST_MAX_GUARD = 64;
constexpr int WALK_THREADS = 1024;
constexpr int WALK_WAVES = WALK_THREADS / WH_WAVE;

// lanes run along f: every row read is one coalesced 256-byte load per wave; the loop over m carries four independent sums
__global__ __launch_bounds__(LEVEL_THREADS) void frame_level_kernel(const float* __restrict__ mel, int n_mels,
                                                                    int64_t frame_stride, int64_t content,
                                                                    float* __restrict__ level) {
  const int64_t f = (int64_t)blockIdx.x * LEVEL_THREADS + threadIdx.x;
  if (f >= content) return;
  const float k = 13.287712379549449f;            // 4 log2(10): 10^(4 M - 4) = 2^(k M - k)
  const float* p = mel + f;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int m = 0;
  for (; m + 4 <= n_mels; m += 4) {
    const float a = p[(int64_t)m * frame_stride], b = p[(int64_t)(m + 1) * frame_stride];
    const float c = p[(int64_t)(m + 2) * frame_stride], d = p[(int64_t)(m + 3) * frame_stride];
    s0 += exp2f(__builtin_fmaf(a, k, -k));
    s1 += exp2f(__builtin_fmaf(b, k, -k));
    s2 += exp2f(__builtin_fmaf(c, k, -k));
    s3 += exp2f(__builtin_fmaf(d, k, -k));
  }
  for (; m < n_mels; ++m) s0 += exp2f(__builtin_fmaf(p[(int64_t)m * frame_stride], k, -k));
  level[f] = log10f(((s0 + s1) + (s2 + s3)) / (float)n_mels);
}

// a tile of L with a halo of W frames on both sides in LDS; frames outside [0, content) hold -inf (they are not in the max)
__global__ __launch_bounds__(COST_TILE) void cut_cost_kernel(const float* __restrict__ level, int64_t content, int W,
                                                             float* __restrict__ cost) {
  __shared__ float tile[COST_TILE + 2 * COST_MAX_GUARD];
  const int64_t base = (int64_t)blockIdx.x * COST_TILE;
  for (int i = threadIdx.x; i < COST_TILE + 2 * W; i += COST_TILE) {
    const int64_t g = base - W + i;
    tile[i] = (g >= 0 && g < content) ? level[g] : -__builtin_huge_valf();
  }
  __syncthreads();
  const int64_t f = base + threadIdx.x;
  if (f >= content) return;
  float best = tile[threadIdx.x];
  for (int j = 1; j <= 2 * W; ++j) {
    const float v = tile[threadIdx.x + j];
    best = v > best ? v : best;
  }
  cost[f] = best;
}

// (value, index) pairs ordered as (value, -index): the smaller value wins, the larger index among equal values
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi > i)) { v = ov; i = oi; }
}

// ONE workgroup: the walk is sequential over chunks, every step is an arg-min over <= max_frames - min_frames + 1 costs
__global__ __launch_bounds__(WALK_THREADS) void cut_walk_kernel(const float* __restrict__ cost, int content, int min_frames,
                                                                int max_frames, int* __restrict__ cuts,
                                                                int* __restrict__ n_cuts, int max_cuts) {
  __shared__ float wave_v[WALK_WAVES];
  __shared__ int wave_i[WALK_WAVES];
  __shared__ int chosen;
  const int tid = threadIdx.x, lane = tid & (WH_WAVE - 1), wave = tid / WH_WAVE;
  int a = 0, n = 0;
  while (content - a > max_frames && n < max_cuts) {
    const int lo = a + min_frames, hi = a + max_frames;     // hi < content: every read below is inside cost[]
    float v = __builtin_huge_valf();
    int idx = -1;
    for (int f = lo + tid; f <= hi; f += WALK_THREADS) take_better(v, idx, cost[f], f);
    for (int off = WH_WAVE / 2; off > 0; off >>= 1)
      take_better(v, idx, __shfl_xor(v, off, WH_WAVE), __shfl_xor(idx, off, WH_WAVE));
    if (lane == 0) { wave_v[wave] = v; wave_i[wave] = idx; }
    __syncthreads();
    if (wave == 0) {
      v = lane < WALK_WAVES ? wave_v[lane] : __builtin_huge_valf();
      idx = lane < WALK_WAVES ? wave_i[lane] : -1;
      for (int off = WALK_WAVES / 2; off > 0; off >>= 1)
        take_better(v, idx, __shfl_xor(v, off, WH_WAVE), __shfl_xor(idx, off, WH_WAVE));
      if (lane == 0) {
        if (idx < lo) idx = hi;                             // no comparable cost in the range (all NaN): cut at the window's end
        chosen = idx;
        cuts[n] = idx;
      }
    }
    __syncthreads();
    a = chosen;
    ++n;
    __syncthreads();                                        // `chosen` and the per-wave slots are rewritten by the next step
  }
  if (tid == 0) *n_cuts = n;
}

}  // namespace

namespace whk {

hipError_t launch_frame_level(const float* mel, int n_mels, int64_t frame_stride, int64_t content, float* level,
                              hipStream_t stream) {
  if (content <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((content + LEVEL_THREADS - 1) / LEVEL_THREADS);
  hipLaunchKernelGGL(frame_level_kernel, dim3(blocks), dim3(LEVEL_THREADS), 0, stream, mel, n_mels, frame_stride, content,
                     level);
  return hipGetLastError();
}

hipError_t launch_speech_cuts(const float* level, int content, int min_frames, int max_frames, int guard, float* cost,
                              int* cuts, int* n_cuts, int max_cuts, hipStream_t stream) {
  if (guard < 0 || guard > COST_MAX_GUARD || content <= 0 || !cost) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)(((int64_t)content + COST_TILE - 1) / COST_TILE);
  hipLaunchKernelGGL(cut_cost_kernel, dim3(blocks), dim3(COST_TILE), 0, stream, level, (int64_t)content, guard, cost);
  hipLaunchKernelGGL(cut_walk_kernel, dim3(1), dim3(WALK_THREADS), 0, stream, (const float*)cost, content, min_frames,
                     max_frames, cuts, n_cuts, max_cuts);
  return hipGetLastError();
}

}  // namespace whk
