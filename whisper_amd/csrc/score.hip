// score.hip — teacher-forced scoring: tied-embedding projection + log-sum-exp + target gather, fused.
//
// For every selected position m the caller wants log softmax(xn[m] · tok_embᵀ)[target[m]] over the first v_end
// vocabulary entries, plus the arg-max and its log-probability.  The logits route (gemm.hip into fp32 [M][V], then a
// softmax and a gather) writes and re-reads M x V x 4 bytes — 1.1 GB for 24 rows x 224 positions of large-v3 — to keep
// M numbers.  Here the [M][V] product never leaves the registers:
//
//   score_slice_kernel   one workgroup per (128-row tile, 128-column vocabulary slice).  The K loop is gemm_nt_kernel's
//                        (gemm.hip): 2 x 2 waves of 64 x 64, K consumed 128 bytes per step through a two-buffer
//                        global_load_lds ring, swizzle on the source address and on the ds_read_b128 fragment reads,
//                        weight fragment as the MFMA's A operand so that a lane ends with 4 consecutive n of one m.
//                        fp16: v_mfma_f32_16x16x32_f16; fp32 (strict engine): v_mfma_f32_16x16x4_f32.
//                        The epilogue reduces the slice per row — max and lowest arg-max (exact), the target's logit if
//                        the slice holds it, then sum exp(logit - slice max) in a fixed order — and writes ONE partial
//                        (max, sumexp, argmax, target logit or -inf) per (row, slice).  Columns >= v_end are masked;
//                        the matrix is not padded (rows beyond V re-read row V - 1 and are masked).
//   score_merge_kernel   one thread per row walks the row's partials in slice order: pass 1 takes the global max /
//                        arg-max / target logit, pass 2 adds sumexp_s * exp(max_s - max).  No atomics anywhere: the
//                        same inputs give the same bits.
//
// Add chain of one log-sum (what the test's fp32 summation bound counts): SCORE_BN / 8 = 16 values per lane, 2
// cross-lane steps, SCORE_WGN - 1 = 1 across the waves of a slice, then one add per slice in the merge.
#include "common.h"
#include "kernels.h"

namespace {

struct ScoreArgs {
  const void* xn; int64_t ldx;      // [M][K] element type
  const void* W; int64_t ldw;       // [V][K]
  const int* target;                // [M]
  float4v* part;                    // [slices][M]: (max, sumexp, argmax bits, target logit or -inf)
  int M, K, V, v_end, tiles_n;
};

constexpr int FM = 4, FN = 4;                    // MFMA 16x16 tiles per wave: a 64x64 block
constexpr int WGM = 2, WGN = whk::SCORE_WGN;     // waves per workgroup
constexpr int BM = WGM * FM * 16, BN = WGN * FN * 16;
static_assert(BN == whk::SCORE_BN, "slice width");
constexpr int NW = WGM * WGN;
constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, STAGE_BYTES = A_BYTES + W_BYTES;
constexpr int RING_BYTES = 2 * STAGE_BYTES;
constexpr int RED_BYTES = 4 * WGN * BM * 4;      // max, argmax, target logit, sumexp: [WGN][BM] words each
constexpr int SCORE_LDS = RING_BYTES + RED_BYTES;
static_assert(SCORE_LDS <= 160 * 1024, "LDS ring + reduction words do not fit");

// (max, lowest index) of two candidates
__device__ __forceinline__ void take_max(float& m, int& i, float om, int oi) {
  if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}

template <typename T>
__global__ __launch_bounds__(NW * 64) void score_slice_kernel(ScoreArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename ET<T>::unit_t unit_t;
  constexpr int UNIT = ET<T>::UNIT;
  constexpr int BKE = 128 / (int)sizeof(T);
  constexpr int IA = BM / (NW * 8), IW = BN / (NW * 8);      // wave-loads (8 rows each) per wave per K step

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;

  // XCD-aware, bijective remap of the linear workgroup id (block b runs on XCD b % 8)
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
  const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
  const int tile_m = wg / p.tiles_n, tile_n = wg - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const T* A = (const T*)p.xn;
  const T* W = (const T*)p.W;

  // staging: instruction i of a wave covers tile rows [(wave*I+i)*8, +8): lane -> row (lane>>3), LDS unit slot (lane&7)
  const T* ga[IA];
  const T* gw[IW];
#pragma unroll
  for (int i = 0; i < IA; ++i) {
    const int r = (wave * IA + i) * 8 + (lane >> 3);
    const int u = (lane & 7) ^ ((r >> 1) & 7);
    int am = m0 + r; if (am > p.M - 1) am = p.M - 1;
    ga[i] = A + (int64_t)am * p.ldx + u * UNIT;
  }
#pragma unroll
  for (int i = 0; i < IW; ++i) {
    const int r = (wave * IW + i) * 8 + (lane >> 3);
    const int u = (lane & 7) ^ ((r >> 1) & 7);
    int wr = n0 + r; if (wr > p.V - 1) wr = p.V - 1;
    gw[i] = W + (int64_t)wr * p.ldw + u * UNIT;
  }

  float4v acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

  // the targets of this lane's rows, requested before the K loop
  int tgt[FM];
#pragma unroll
  for (int tm = 0; tm < FM; ++tm) {
    const int m = m0 + wm * (FM * 16) + tm * 16 + (lane & 15);
    tgt[tm] = p.target[m < p.M ? m : p.M - 1];
  }

  const int nk = p.K / BKE;
  auto stage = [&](int buf, int kt) {
    char* sA = smem + buf * STAGE_BYTES + (wave * IA) * 1024;
    char* sW = smem + buf * STAGE_BYTES + A_BYTES + (wave * IW) * 1024;
    const int64_t ko = (int64_t)kt * BKE;
#pragma unroll
    for (int i = 0; i < IA; ++i) glds16(ga[i] + ko, sA + i * 1024);
#pragma unroll
    for (int i = 0; i < IW; ++i) glds16(gw[i] + ko, sW + i * 1024);
  };

  // two tile buffers, ONE barrier per K step: wait for my loads of tile kt, barrier (=> every wave sees tile kt AND has
  // finished reading tile kt-1), refill tile kt-1's buffer with tile kt+1, then the MFMAs of tile kt run meanwhile
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    const char* sA = smem + (kt & 1) * STAGE_BYTES;
    const char* sW = sA + A_BYTES;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      unit_t af[FM], wf[FN];
      const int u = 4 * q + (lane >> 4);
#pragma unroll
      for (int t = 0; t < FM; ++t) af[t] = *(const unit_t*)(sA + swz_byte(wm * (FM * 16) + t * 16 + (lane & 15), u));
#pragma unroll
      for (int t = 0; t < FN; ++t) wf[t] = *(const unit_t*)(sW + swz_byte(wn * (FN * 16) + t * 16 + (lane & 15), u));
#pragma unroll
      for (int tn = 0; tn < FN; ++tn)
#pragma unroll
        for (int tm = 0; tm < FM; ++tm) mma16(wf[tn], af[tm], acc[tn][tm]);
    }
  }

  // ---- epilogue: lane holds logit[m][n..n+3] for m = m0+wm*64+tm*16+(lane&15), n = n0+wn*64+tn*16+(lane>>4)*4.
  // The reduction words live behind the ring, so no wave still reading the last K tile is disturbed.
  float* red_max = (float*)(smem + RING_BYTES);
  int* red_idx = (int*)(red_max + WGN * BM);
  float* red_tgt = (float*)(red_idx + WGN * BM);
  float* red_sum = red_tgt + WGN * BM;
  const int ncol0 = n0 + wn * (FN * 16) + (lane >> 4) * 4;

#pragma unroll
  for (int tm = 0; tm < FM; ++tm) {
    float lmax = WH_NEG_INF, ltgt = WH_NEG_INF;
    int lidx = 0x7fffffff;
#pragma unroll
    for (int tn = 0; tn < FN; ++tn)
#pragma unroll
      for (int e = 0; e < 4; ++e) {                // ascending n: a strict > keeps the lowest index
        const int n = ncol0 + tn * 16 + e;
        const float v = acc[tn][tm][e];
        if (n < p.v_end) {
          if (v > lmax) { lmax = v; lidx = n; }
          if (n == tgt[tm]) ltgt = v;
        }
      }
    // the four lane groups of a row: lanes l, l^16, l^32, l^48
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
      const float om = __shfl_xor(lmax, d);
      const int oi = __shfl_xor(lidx, d);
      const float ot = __shfl_xor(ltgt, d);
      take_max(lmax, lidx, om, oi);
      ltgt = fmaxf(ltgt, ot);
    }
    if (lane < 16) {
      const int ml = wm * (FM * 16) + tm * 16 + lane;
      red_max[wn * BM + ml] = lmax; red_idx[wn * BM + ml] = lidx; red_tgt[wn * BM + ml] = ltgt;
    }
  }
  __syncthreads();

  float gmax[FM], gtgt[FM];
  int gidx[FM];
#pragma unroll
  for (int tm = 0; tm < FM; ++tm) {
    const int ml = wm * (FM * 16) + tm * 16 + (lane & 15);
    gmax[tm] = WH_NEG_INF; gtgt[tm] = WH_NEG_INF; gidx[tm] = 0x7fffffff;
#pragma unroll
    for (int w = 0; w < WGN; ++w) {
      take_max(gmax[tm], gidx[tm], red_max[w * BM + ml], red_idx[w * BM + ml]);
      gtgt[tm] = fmaxf(gtgt[tm], red_tgt[w * BM + ml]);
    }
    // sum exp(logit - slice max): 16 values of the lane in ascending n, two cross-lane steps, then the waves in order
    float lsum = 0.f;
#pragma unroll
    for (int tn = 0; tn < FN; ++tn)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = ncol0 + tn * 16 + e;
        lsum += (n < p.v_end) ? expf(acc[tn][tm][e] - gmax[tm]) : 0.f;
      }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (lane < 16) red_sum[wn * BM + wm * (FM * 16) + tm * 16 + lane] = lsum;
  }
  __syncthreads();

  if (wn == 0 && lane < 16) {
#pragma unroll
    for (int tm = 0; tm < FM; ++tm) {
      const int ml = wm * (FM * 16) + tm * 16 + lane;
      const int m = m0 + ml;
      float s = red_sum[ml];
#pragma unroll
      for (int w = 1; w < WGN; ++w) s += red_sum[w * BM + ml];
      if (m < p.M) p.part[(int64_t)tile_n * p.M + m] = float4v{gmax[tm], s, __int_as_float(gidx[tm]), gtgt[tm]};
    }
  }
}

// one thread per row, the row's partials in slice order
__global__ __launch_bounds__(64) void score_merge_kernel(const float4v* part, const int* target, int M, int slices,
                                                         float* logprob, float* top_logprob, int* top_token) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  if (target[m] < 0) {                                   // padded slot
    logprob[m] = 0.f;
    if (top_logprob) top_logprob[m] = 0.f;
    if (top_token) top_token[m] = -1;
    return;
  }
  float gmax = WH_NEG_INF, gtgt = WH_NEG_INF;
  int gidx = 0x7fffffff;
  for (int s = 0; s < slices; ++s) {
    const float4v q = part[(int64_t)s * M + m];
    take_max(gmax, gidx, q[0], __float_as_int(q[2]));
    gtgt = fmaxf(gtgt, q[3]);
  }
  float sum = 0.f;
  for (int s = 0; s < slices; ++s) {
    const float4v q = part[(int64_t)s * M + m];
    sum += q[1] * expf(q[0] - gmax);
  }
  const float ls = logf(sum);                            // sum >= 1: the maximum's own term
  logprob[m] = (gtgt - gmax) - ls;                       // -inf when no slice below v_end held the target
  if (top_logprob) top_logprob[m] = -ls;
  if (top_token) top_token[m] = gidx;
}

// target[r][i] = tokens[r][first + i + 1], or -1 where that token lies beyond the row's valid length
__global__ void score_targets_kernel(const int64_t* tokens, int64_t token_stride, const int* n_tok, int R, int n_out,
                                     int first, int* target) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * n_out) return;
  const int r = i / n_out, p = first + (i - r * n_out);
  target[i] = (p + 1 < n_tok[r]) ? (int)tokens[r * token_stride + p + 1] : -1;
}

template <typename T>
hipError_t launch_slices(const ScoreArgs& p, hipStream_t stream) {
  static whk::LdsAttr attr;
  { hipError_t e = whk::raise_dynamic_lds(attr, (const void*)score_slice_kernel<T>, SCORE_LDS); if (e != hipSuccess) return e; }
  const int tiles_m = (p.M + BM - 1) / BM;
  hipLaunchKernelGGL((score_slice_kernel<T>), dim3(tiles_m * p.tiles_n), dim3(NW * 64), SCORE_LDS, stream, p);
  return hipGetLastError();
}

}  // namespace

namespace whk {

size_t score_scratch_bytes(int64_t M, int V) {
  if (M <= 0 || V <= 0) return 0;
  return (size_t)((V + SCORE_BN - 1) / SCORE_BN) * (size_t)M * 16;
}

hipError_t launch_score(const void* xn, int64_t ldx, const void* W, int64_t ldw, const int* target, int M, int K, int V,
                        int v_end, float* logprob, float* top_logprob, int* top_token, void* scratch,
                        size_t scratch_bytes, int dtype, hipStream_t stream) {
  const int bke = dtype == 1 ? 64 : 32;
  if (!xn || !W || !target || !logprob || !scratch || (((uintptr_t)scratch) & 15)) return hipErrorInvalidValue;
  if (M <= 0 || K <= 0 || K % bke != 0 || V <= 0 || v_end < 1 || v_end > V) return hipErrorInvalidValue;
  if (ldx < K || ldw < K || (ldx * (dtype == 1 ? 2 : 4)) % 16 || (ldw * (dtype == 1 ? 2 : 4)) % 16) return hipErrorInvalidValue;
  ScoreArgs p;
  p.xn = xn; p.ldx = ldx; p.W = W; p.ldw = ldw; p.target = target; p.part = (float4v*)scratch;
  p.M = M; p.K = K; p.V = V; p.v_end = v_end;
  p.tiles_n = (v_end + SCORE_BN - 1) / SCORE_BN;          // slices that hold a column below v_end
  if ((size_t)p.tiles_n * (size_t)M * 16 > scratch_bytes) return hipErrorInvalidValue;
  if ((int64_t)((M + BM - 1) / BM) * p.tiles_n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipError_t e = dtype == 1 ? launch_slices<half_t>(p, stream) : launch_slices<float>(p, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_merge_kernel, dim3((M + 63) / 64), dim3(64), 0, stream, p.part, target, M, p.tiles_n, logprob,
                     top_logprob, top_token);
  return hipGetLastError();
}

hipError_t launch_score_targets(const int64_t* tokens, int64_t token_stride, const int* n_tok, int R, int n_out, int first,
                                int* target, hipStream_t stream) {
  const int n = R * n_out;
  hipLaunchKernelGGL(score_targets_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tokens, token_stride, n_tok, R,
                     n_out, first, target);
  return hipGetLastError();
}

}  // namespace whk
