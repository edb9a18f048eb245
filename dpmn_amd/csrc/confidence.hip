// Recogniser confidence (ours; main.py --demo_conf / --demo_upright / --demo_min_conf, utils/confidence.py is the NumPy restatement).
//   k_ctc_conf   per image the CTC log-likelihood of ITS OWN greedy string (the output of k_ctc_greedy) under its frame posteriors:
//                the forward / alpha recursion of lexicon.hip with the word taken from cls / len instead of a record, any length
//                0 <= n <= T (up to 2 T + 1 = 129 states, one to three per lane)
//   k_attn_conf  per image the sum of log_softmax(logits[t])[ids[t]] over the steps up to and with the first EOS, and their count
//   k_turn180    the 180 degree turn of every plane of an NCHW batch
// The row log-sum-exps are taken in fp64 (one exp per class and frame: nothing beside the recogniser's forward), so that a score of
// one or two factors is as good as its fp32 rounding; the recursion itself is fp32 in the log domain, max-shifted.
// No kernel has a matrix product or a variant per compute mode.
#include "common.h"

namespace {

constexpr int CF_MAX_T = 64;         // frames (the lexicon kernel's limits)
constexpr int CF_MAX_C = 64;         // classes
constexpr int CF_LD = CF_MAX_C + 1;  // LDS row: lane = frame walks its row without a bank conflict
constexpr int AT_MAX = 128;          // attention decoders: steps and classes

// v of lane - 1 (wave_shr:1 crosses the rows of 16); lane 0 keeps `first`
__device__ __forceinline__ float lane_below(float first, float v) {
  return __uint_as_float(dpp_mov_u<0x138, 0xF>(__float_as_uint(first), __float_as_uint(v)));
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// log(e^a + e^b + e^c); -inf when all three are
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += xshfl_v(v, o);
  return v;
}

// The alpha recursion with K states per lane: state s = 64 k + lane, label = blank for even s, lab[(s - 1) / 2] for odd s; a skip
// over the blank only between different labels.  States >= 2 n + 1 run along: a state only feeds higher states.
// -> log(alpha[2n] + alpha[2n - 1]) after the last frame.
template <int K>
__device__ __forceinline__ float ctc_alpha(const float* lp, const int* lab, int n, int T, int lane) {
  int label[K];
  bool skip[K];
  float a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = 64 * k + lane;
    const bool sym = (s & 1) && s < 2 * n + 1;
    label[k] = sym ? lab[s >> 1] : 0;
    skip[k] = sym && s >= 3 && label[k] != lab[(s >> 1) - 1];
    a[k] = s == 0 ? lp[0] : (s == 1 && n > 0 ? lp[label[k]] : -INFINITY);
  }
  for (int t = 1; t < T; ++t) {
    float p1[K], p2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) p1[k] = lane_below(k > 0 ? lane_value(a[k > 0 ? k - 1 : 0], 63) : -INFINITY, a[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) p2[k] = lane_below(k > 0 ? lane_value(p1[k > 0 ? k - 1 : 0], 63) : -INFINITY, p1[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = lse3(a[k], p1[k], skip[k] ? p2[k] : -INFINITY) + lp[t * CF_LD + label[k]];
  }
  float last = -INFINITY, prev = -INFINITY;
  const int sl = 2 * n, sp = 2 * n - 1;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if ((sl >> 6) == k) last = lane_value(a[k], sl & 63);
    if (sp >= 0 && (sp >> 6) == k) prev = lane_value(a[k], sp & 63);
  }
  return lse3(last, prev, -INFINITY);
}

// grid (B), one wave.  logits: rows b*T + t, leading dimension ld, columns >= n_class never read.  cls (B, T), len (B): k_ctc_greedy's.
// Phase 0: the image's logits into LDS (lane = class).  Phase 1: lane = frame: its row's log-sum-exp in fp64, the row -> log-softmax.
// Phase 2: the recursion, lane = state (DPP neighbours, no barrier inside the T loop); one, two or three states per lane by n.
__global__ __launch_bounds__(64) void k_ctc_conf(const float* __restrict__ logits, int ld, int n_class, const int* __restrict__ cls,
                                                  const int* __restrict__ len, float* __restrict__ out, int T) {
  __shared__ float lp[CF_MAX_T * CF_LD];
  __shared__ int lab[CF_MAX_T];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane < n_class)
    for (int t = 0; t < T; ++t) lp[t * CF_LD + lane] = logits[((size_t)b * T + t) * ld + lane];
  const int n = min(max(__builtin_amdgcn_readfirstlane(len[b]), 0), T);
  lab[lane] = lane < n ? min(max(cls[(size_t)b * T + lane], 0), n_class - 1) : 0;   // (a bad class stays inside the row)
  __syncthreads();
  if (lane < T) {
    float* r = lp + lane * CF_LD;
    float m = r[0];
    for (int c = 1; c < n_class; ++c) m = fmaxf(m, r[c]);
    double sum = 0.0;
    for (int c = 0; c < n_class; ++c) sum += exp((double)r[c] - (double)m);
    const double ls = log(sum);                                  // (x - m) - log(sum): a margin of 40 keeps the log-probability e^-40
    for (int c = 0; c < n_class; ++c) r[c] = (float)(((double)r[c] - (double)m) - ls);
  }
  __syncthreads();
  float s;
  if (2 * n + 1 <= 64) s = ctc_alpha<1>(lp, lab, n, T, lane);
  else if (2 * n + 1 <= 128) s = ctc_alpha<2>(lp, lab, n, T, lane);
  else s = ctc_alpha<3>(lp, lab, n, T, lane);
  if (lane == 0) out[b] = s;
}

// grid (B), one wave, lane = class (and class + 64).  logits (B, steps, n_class), ids (B, steps).
__global__ __launch_bounds__(64) void k_attn_conf(const float* __restrict__ logits, const int* __restrict__ ids, int eos,
                                                   float* __restrict__ out_score, int* __restrict__ out_terms, int steps, int n_class) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* id = ids + (size_t)b * steps;
  // the summed steps: up to and with the first EOS
  const unsigned long long e0 = __ballot(lane < steps && id[lane] == eos);
  const unsigned long long e1 = __ballot(lane + 64 < steps && id[min(lane + 64, steps - 1)] == eos);
  const int terms = e0 ? __ffsll((long long)e0) : (e1 ? 64 + __ffsll((long long)e1) : steps);
  double score = 0.0;
  for (int t = 0; t < terms; ++t) {
    const float* r = logits + ((size_t)b * steps + t) * n_class;
    const float x0 = lane < n_class ? r[lane] : -INFINITY;
    const float x1 = lane + 64 < n_class ? r[lane + 64] : -INFINITY;
    const float m = wave_max(fmaxf(x0, x1));
    double e = lane < n_class ? exp((double)x0 - (double)m) : 0.0;
    if (lane + 64 < n_class) e += exp((double)x1 - (double)m);
    const double sum = wave_sum_d(e);
    const int c = min(max(__builtin_amdgcn_readfirstlane(id[t]), 0), n_class - 1);   // (a bad id stays inside the row)
    score += ((double)r[c] - (double)m) - log(sum);
  }
  if (lane == 0) {
    out_score[b] = (float)score;
    out_terms[b] = terms;
  }
}

// one element per thread: y[plane][hw - 1 - i] = x[plane][i] (rows and columns reversed = the flat plane reversed)
__global__ void k_turn180(const float* __restrict__ x, float* __restrict__ y, long total, long hw) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long p = idx / hw, i = idx - p * hw;
  y[p * hw + (hw - 1 - i)] = x[idx];
}

}  // namespace

extern "C" {

int dpmn_ctc_conf_f32(const float* logits, int ld, int n_class, const int* cls, const int* len, float* out_score, int B, int T,
                      dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && cls && len && out_score && B > 0 && T > 0 && n_class > 0 && ld >= n_class, "ctc_conf: bad arguments");
  DPMN_REQUIRE(T <= CF_MAX_T && n_class <= CF_MAX_C, "ctc_conf: at most 64 frames and 64 classes");
  hipLaunchKernelGGL(k_ctc_conf, dim3((unsigned)B), dim3(64), 0, as_stream(stream), logits, ld, n_class, cls, len, out_score, T);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_attn_conf_f32(const float* logits, const int* ids, int eos, float* out_score, int* out_terms, int B, int steps, int n_class,
                       dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && ids && out_score && out_terms && B > 0 && steps > 0 && n_class > 0, "attn_conf: bad arguments");
  DPMN_REQUIRE(steps <= AT_MAX && n_class <= AT_MAX, "attn_conf: at most 128 steps and 128 classes");
  hipLaunchKernelGGL(k_attn_conf, dim3((unsigned)B), dim3(64), 0, as_stream(stream), logits, ids, eos, out_score, out_terms, steps, n_class);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_turn180_f32(const float* x, float* y, int B, int C, int H, int W, dpmn_stream_t stream) {
  DPMN_REQUIRE(x && y && x != y && B > 0 && C > 0 && H > 0 && W > 0, "turn180: bad arguments");
  const long hw = (long)H * W, total = hw * B * C;
  DPMN_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "turn180: the batch is too large for one launch");
  hipLaunchKernelGGL(k_turn180, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, total, hw);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
