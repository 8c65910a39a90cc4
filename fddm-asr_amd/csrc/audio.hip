// Audio front end of the inference entry point: interleaved multi-channel f32 samples at any source rate -> 16 kHz
// mono rows of a padded batch, in one launch per source rate (include/fddm_hip.h: fddm_wav_resample).
//
// The filter is torchaudio.functional.resample's Hann-windowed sinc (fddm_hip/audio.py builds the table in float64):
// output j of an utterance is the dot product of phase row j % P with the KT mono frames starting at (j / P) * Q - W.
// Most of a large-ratio table is zero (the window's clamped region), so the kernel takes the table compacted: per phase
// the NT consecutive taps from klo[p] on, stored [NT][P] so that lanes on consecutive phases read consecutive floats.
//
// One workgroup per (utterance, OB consecutive outputs): the block's mono input span is staged in LDS with the channel
// mean done on the way in (16-byte loads for mono and stereo where the span is inside the clip), then each lane
// accumulates its outputs from LDS in tap order. Frames outside [0, n) are zeros; outputs from n_out on are zeros.
#include "common.h"

#include <algorithm>
#include <vector>

namespace fddm {
namespace audio {

constexpr int OB = 1024;       // outputs per workgroup
constexpr int NTHR = 256;
constexpr int MAXU = 64;       // utterances per launch (descriptors travel as a kernel argument)
constexpr long LDS_MAX = 65536;

struct Utt {
  long off;   // first float of the clip in src
  int n;      // frames
  int nch;    // channels, 1..8
  int row;    // destination row of wave / lengths
  int pad;
};
struct Batch {
  Utt u[MAXU];
};

// channel mean of 4 consecutive frames whose first float is 16-byte aligned: NCH float4 loads, one float4 LDS write
template <int NCH> __device__ __forceinline__ float4 mean4(const float* g) {
  float e[4 * NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float4 v = ((const float4*)g)[c];
    e[4 * c] = v.x, e[4 * c + 1] = v.y, e[4 * c + 2] = v.z, e[4 * c + 3] = v.w;
  }
  float m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s = e[i * NCH];
#pragma unroll
    for (int c = 1; c < NCH; ++c) s += e[i * NCH + c];
    m[i] = s / (float)NCH;
  }
  return make_float4(m[0], m[1], m[2], m[3]);
}

__device__ __forceinline__ float mean1(const float* clip, long f, int n, int nch) {
  if (f < 0 || f >= n) return 0.f;
  const float* p = clip + f * nch;
  float s = p[0];
  for (int c = 1; c < nch; ++c) s += p[c];
  return s / (float)nch;
}

// frames fa .. fa + cnt - 1 (fa, cnt multiples of 4) of the clip's channel mean into lds[0 .. cnt)
template <int NCH> __device__ __forceinline__ void stage(const float* clip, long fa, int cnt, int n, int nch, float* lds) {
  for (int g = threadIdx.x; g < cnt / 4; g += NTHR) {
    const long f = fa + 4L * g;
    float4 m;
    if (NCH && f >= 0 && f + 3 < n)
      m = mean4<NCH ? NCH : 1>(clip + f * NCH);
    else
      m = make_float4(mean1(clip, f, n, nch), mean1(clip, f + 1, n, nch), mean1(clip, f + 2, n, nch),
                      mean1(clip, f + 3, n, nch));
    ((float4*)lds)[g] = m;
  }
}

__global__ __launch_bounds__(NTHR) void wav_resample_kernel(const float* __restrict__ src, const Batch batch,
                                                           const float* __restrict__ taps, const int* __restrict__ klo,
                                                           int NT, int P, int Q, int W, float* __restrict__ wave,
                                                           long* __restrict__ lengths, int T) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Utt u = batch.u[blockIdx.y];
  const int KT = 2 * W + Q;
  const long full = ((long)u.n * P + Q - 1) / Q;
  const int n_out = (int)(full < (long)T ? full : (long)T);
  const int j0 = blockIdx.x * OB;
  const int jend = min(j0 + OB, n_out);   // outputs [j0, jend) are computed, [jend, min(j0 + OB, T)) are zeros
  if (blockIdx.x == 0 && threadIdx.x == 0) lengths[u.row] = n_out;
  float* out = wave + (long)u.row * T;
  long fa = 0;
  if (jend > j0) {   // block-uniform
    const long f0 = (long)(j0 / P) * Q - W;
    fa = f0 & ~3L;   // floor to a multiple of 4, negative f0 included
    const int cnt = (int)((long)((jend - 1) / P) * Q - W + KT - fa + 3) & ~3;
    const float* clip = src + u.off;
    const bool vec = ((u.off & 3) == 0) && ((((uintptr_t)src) & 15) == 0);
    if (vec && u.nch == 1)
      stage<1>(clip, fa, cnt, u.n, 1, lds);
    else if (vec && u.nch == 2)
      stage<2>(clip, fa, cnt, u.n, 2, lds);
    else
      stage<0>(clip, fa, cnt, u.n, u.nch, lds);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < OB / NTHR; ++i) {
    const int j = j0 + i * NTHR + (int)threadIdx.x;
    if (j >= T) break;
    float acc = 0.f;
    if (j < jend) {
      const int q = j / P, p = j - q * P;
      const int kl = min(max(klo[p], 0), KT - NT);
      const float* x = lds + ((long)q * Q - W - fa) + kl;
      const float* h = taps + p;
      for (int k = 0; k < NT; ++k) acc = fmaf(h[(long)k * P], x[k], acc);
    }
    out[j] = acc;
  }
}

}  // namespace audio
}  // namespace fddm

using namespace fddm::audio;

FDDM_API int fddm_wav_resample(const float* src, long src_len, const long* desc, long B, const float* taps,
                               const int* klo, int NT, int P, int Q, int W, float* wave, long* lengths, long rows,
                               long T, void* hs) {
  if (B <= 0) return 0;
  if (!desc || !taps || !klo || !wave || !lengths || src_len < 0 || (!src && src_len > 0)) return (int)hipErrorInvalidValue;
  if (P < 1 || Q < 1 || W < 0 || NT < 1 || (long)NT > 2L * W + Q) return (int)hipErrorInvalidValue;
  if (rows < 1 || rows > 0x7fffffffL || T < 1 || T > 0x7fffffffL - OB) return (int)hipErrorInvalidValue;
  // the block's mono span: at most ((OB - 1) / P + 1) * Q + KT frames, plus the round-down of its start and the
  // round-up of its length to multiples of 4
  const long lds_bytes = ((long)((OB - 1) / P + 1) * Q + 2L * W + Q + 3 + 3) / 4 * 16;
  if (lds_bytes > LDS_MAX) return (int)hipErrorInvalidValue;
  for (long b = 0; b < B; ++b) {
    const long off = desc[4 * b], n = desc[4 * b + 1], nch = desc[4 * b + 2], row = desc[4 * b + 3];
    if (off < 0 || off > src_len || n < 0 || n > 0x7fffffffL / P || nch < 1 || nch > 8 || row < 0 || row >= rows)
      return (int)hipErrorInvalidValue;
    if (n * nch > src_len - off) return (int)hipErrorInvalidValue;
  }
  {  // two clips on one row would race on it
    std::vector<long> r((size_t)B);
    for (long b = 0; b < B; ++b) r[(size_t)b] = desc[4 * b + 3];
    std::sort(r.begin(), r.end());
    if (std::adjacent_find(r.begin(), r.end()) != r.end()) return (int)hipErrorInvalidValue;
  }
  for (long b0 = 0; b0 < B; b0 += MAXU) {
    const int nb = (int)(B - b0 < MAXU ? B - b0 : MAXU);
    Batch bt = {};
    for (int i = 0; i < nb; ++i) {
      const long* d = desc + 4 * (b0 + i);
      bt.u[i].off = d[0], bt.u[i].n = (int)d[1], bt.u[i].nch = (int)d[2], bt.u[i].row = (int)d[3];
    }
    hipLaunchKernelGGL(wav_resample_kernel, dim3((unsigned)((T + OB - 1) / OB), (unsigned)nb), dim3(NTHR),
                       (size_t)lds_bytes, (hipStream_t)hs, src, bt, taps, klo, NT, P, Q, W, wave, lengths, (int)T);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}
