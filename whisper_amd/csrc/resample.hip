// resample.hip — device-side audio ingest (load_audio(..., device=gpu); DESIGN.md §5b "Device-side ingest"): interleaved PCM as a
//   WAV / FLAC reader holds it -> mono float32 at the target rate, already on the 16-bit grid.  One launch does the equal-weight
//   down-mix, the polyphase resampling and the quantisation of the host path (audio.py::_to_mono_s16), in float64:
//     mono[k] = (sum over channels of pcm[k][c]) / (channels * full_scale)                       0 <= k < n_frames
//     y[m]    = sum_k taps[m * down - k * up + half] * mono[k]      (|m * down - k * up| <= half)  0 <= m < n_out
//     out[m]  = clip(rint(32768 y[m]), -32768, 32767) / 32768                                    (rint: half to even)
//   mono outside [0, n_frames) is zero.  taps (2 * half + 1 float64, centre at index half) is scipy's resample_poly filter,
//   built by audio.resample_taps; up == down == 1 with the one tap 1.0 is "down-mix and quantise only".
//   A workgroup owns a run of consecutive outputs, stages the down-mixed span of input frames they reach in LDS once, then
//   output m walks its own phase of the table: tap index q, q + up, q + 2 up, ... with q = (m * down + half) mod up against
//   frames k_hi, k_hi - 1, ... with k_hi = (m * down + half) div up.  About 20 * max(up, down) / up + 1 FMAs per output
//   (56 from 44.1 kHz); the arithmetic is not the cost, so nothing is traded for it.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_SPAN = 4096;                       // float64 frames of LDS per workgroup (32 KB)

template <typename T> struct Pcm {                  // exact channel sum for the integer formats
  using Sum = long long;
  static __device__ __forceinline__ Sum zero() { return 0; }
  static __device__ __forceinline__ Sum get(const T* p) { return (Sum)*p; }
};
template <> struct Pcm<uint8_t> {                   // 8-bit WAV: offset binary
  using Sum = long long;
  static __device__ __forceinline__ Sum zero() { return 0; }
  static __device__ __forceinline__ Sum get(const uint8_t* p) { return (Sum)*p - 128; }
};
template <> struct Pcm<float> {
  using Sum = double;
  static __device__ __forceinline__ Sum zero() { return 0.0; }
  static __device__ __forceinline__ Sum get(const float* p) { return (double)*p; }
};
template <> struct Pcm<double> {
  using Sum = double;
  static __device__ __forceinline__ Sum zero() { return 0.0; }
  static __device__ __forceinline__ Sum get(const double* p) { return *p; }
};

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {      // b > 0
  const int64_t q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// per_wg <= RS_THREADS outputs per workgroup, chosen by the launcher so that their span fits RS_SPAN
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const T* __restrict__ pcm, int channels, double denom,
                                                              int64_t n_frames, const double* __restrict__ taps, int up,
                                                              int down, int half, float* __restrict__ out, int64_t n_out,
                                                              int per_wg) {
  __shared__ double span[RS_SPAN];
  const int64_t m0 = (int64_t)blockIdx.x * per_wg;
  const int64_t m_last = (m0 + per_wg < n_out ? m0 + per_wg : n_out) - 1;
  // frames reached by outputs m0 .. m_last: ceil((m0 * down - half) / up) .. floor((m_last * down + half) / up)
  const int64_t k_lo = -floor_div((int64_t)half - m0 * down, up);
  const int64_t k_end = floor_div(m_last * down + half, up);
  const int n_span = (int)(k_end - k_lo + 1);       // <= RS_SPAN (launcher)
  for (int s = threadIdx.x; s < n_span; s += RS_THREADS) {
    const int64_t k = k_lo + s;
    double v = 0.0;
    if (k >= 0 && k < n_frames) {
      const T* p = pcm + k * channels;
      typename Pcm<T>::Sum sum = Pcm<T>::zero();
      for (int c = 0; c < channels; ++c) sum += Pcm<T>::get(p + c);
      v = (double)sum / denom;
    }
    span[s] = v;
  }
  __syncthreads();
  const int64_t m = m0 + threadIdx.x;
  if ((int)threadIdx.x >= per_wg || m > m_last) return;
  const int64_t c = m * down + half;
  int idx = (int)(c % up);                          // c >= 0
  int s = (int)(c / up - k_lo);                     // k_hi - k_lo, inside [0, n_span)
  const int n_taps = 2 * half + 1;
  double acc = 0.0;
  for (; idx < n_taps; idx += up, --s) acc = __builtin_fma(taps[idx], span[s], acc);   // s ends at ceil((m down - half) / up) - k_lo >= 0
  double q = __builtin_rint(acc * 32768.0);
  q = q < -32768.0 ? -32768.0 : (q > 32767.0 ? 32767.0 : q);                            // a NaN stays a NaN, as numpy.clip leaves it
  out[m] = (float)(q * (1.0 / 32768.0));
}

}  // namespace

namespace whk {

int resample_outputs_per_wg(int up, int down, int half) {
  // span of T outputs <= ((T - 1) * down + 2 * half) / up + 2 frames
  const int64_t room = ((int64_t)RS_SPAN - 2) * up - 2 * (int64_t)half;
  if (room < 0) return 0;                           // not even one output's taps fit
  const int64_t t = room / down + 1;
  return t > RS_THREADS ? RS_THREADS : (int)t;
}

hipError_t launch_resample(const void* pcm, int format, int bits, int channels, int64_t n_frames, const double* taps, int up,
                           int down, int half, float* out, int64_t n_out, hipStream_t stream) {
  if (n_out <= 0) return hipSuccess;
  const int per_wg = resample_outputs_per_wg(up, down, half);
  if (per_wg < 1) return hipErrorInvalidValue;
  const int64_t blocks = (n_out + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(RS_THREADS);
  const double scale = format <= 2 ? (format == 0 ? 128.0 : __builtin_ldexp(1.0, bits - 1)) : 1.0;
  const double denom = scale * channels;
  switch (format) {
    case 0: hipLaunchKernelGGL(resample_kernel<uint8_t>, grid, block, 0, stream, (const uint8_t*)pcm, channels, denom, n_frames,
                               taps, up, down, half, out, n_out, per_wg); break;
    case 1: hipLaunchKernelGGL(resample_kernel<int16_t>, grid, block, 0, stream, (const int16_t*)pcm, channels, denom, n_frames,
                               taps, up, down, half, out, n_out, per_wg); break;
    case 2: hipLaunchKernelGGL(resample_kernel<int32_t>, grid, block, 0, stream, (const int32_t*)pcm, channels, denom, n_frames,
                               taps, up, down, half, out, n_out, per_wg); break;
    case 3: hipLaunchKernelGGL(resample_kernel<float>, grid, block, 0, stream, (const float*)pcm, channels, denom, n_frames,
                               taps, up, down, half, out, n_out, per_wg); break;
    case 4: hipLaunchKernelGGL(resample_kernel<double>, grid, block, 0, stream, (const double*)pcm, channels, denom, n_frames,
                               taps, up, down, half, out, n_out, per_wg); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace whk
