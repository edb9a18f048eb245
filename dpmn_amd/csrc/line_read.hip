// One read per tiled text line (ours; main.py --demo_line_read, utils/line_read.py is the NumPy restatement and gives the definition).
//   k_line_stitch  the frame posteriors of a line's overlapping windows -> one log-posterior row per LINE frame: per covering window
//                  the log-softmax of its two neighbouring frames, interpolated, blended over the windows with the pixel stitch's
//                  ramp in the log domain, renormalised.  One wave per line frame, lane = class.
//   k_line_greedy  per line the arg-max classes with repeats collapsed and blanks dropped, and per kept symbol the first and the last
//                  frame of its arg-max run.  One block per line.
//   k_line_ctc     per line the CTC log-likelihood of ITS OWN greedy string: the alpha recursion of k_ctc_conf (confidence.hip) over up
//                  to 3201 frames and 6403 states, the states spread over the block's threads, one to seven per thread.
// The log-sum-exps, the interpolation and the blend of k_line_stitch are fp64, rounded to fp32 once (k_ctc_conf's choice for its row
// sums); the recursion is fp32 in the log domain, max-shifted.  No kernel has a matrix product or a variant per compute mode.
#include "common.h"

namespace {

constexpr int LR_MAX_T = 64;                  // frames per window
constexpr int LR_MAX_C = 64;                  // classes: lane = class
constexpr int LR_MAX_L = 3201;                // frames per line: 8192 columns at 25 frame steps per 64 columns
constexpr int LR_MAX_S = 2 * LR_MAX_L + 1;    // states of the recursion
constexpr int LR_MAX_W = 8192;                // columns per window (utils.resize.MAX_SIDE): j * lr_w and x0 * D stay far inside int
constexpr int LR_MAX_K = 7;                   // states per thread of a block of 1024: 7 * 1024 >= LR_MAX_S

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += xshfl_v(v, o);
  return v;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, xshfl_v(v, o));
  return v;
}

// log(e^a + e^b + e^c); -inf when all three are
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// log_softmax of one window frame (lane = class) in fp64: (x - m) - log(sum e^(x - m)); 0 in the lanes >= n_class
__device__ __forceinline__ double frame_lp(const float* __restrict__ row, int n_class, int lane) {
  const bool on = lane < n_class;
  const float x = on ? row[lane] : -INFINITY;
  const float m = wave_max(x);
  const double d = on ? (double)x - (double)m : 0.0;
  const double sum = wave_sum_d(on ? exp(d) : 0.0);
  return on ? d - log(sum) : 0.0;
}

// grid (ceil(max L / 4), B), 256 threads: wave = line frame j, lane = class.  logits: rows w*T + t, leading dimension ld, columns >=
// n_class never read.  lines (B, 2) [first row of line_lp, L], wins (B, 2) [first window, windows], x0 per window (they do not decrease
// within a line).  With D = T - 1, P = lr_w: num = j P - x0 D; covered iff 0 <= num <= D P; f = num / P, r = num % P (r == 0 reads
// frame f alone: f = D never reads past the window); weight min(num + P, D P - num + P, cap), the line's outer edges at cap = D P / 2.
__global__ __launch_bounds__(256) void k_line_stitch(const float* __restrict__ logits, int ld, int n_class, int T, int P,
                                                      const int* __restrict__ lines, const int* __restrict__ wins,
                                                      const int* __restrict__ x0, float* __restrict__ line_lp) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int j = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int frame0 = lines[2 * b], L = lines[2 * b + 1];
  if (j >= L) return;                                              // (no barrier in this kernel)
  const int first = wins[2 * b], last = first + wins[2 * b + 1] - 1;
  const int D = T - 1, DP = D * P, cap = DP / 2;
  double acc = 0.0;
  long long gsum = 0;
  for (int w = first; w <= last; ++w) {
    const int num = j * P - x0[w] * D;
    if (num < 0) break;                                            // the later windows start further right
    if (num > DP) continue;
    const int f = num / P, r = num - f * P;
    const int g = min(min(w == first ? cap : num + P, w == last ? cap : DP - num + P), cap);
    const float* row = logits + ((size_t)w * T + f) * ld;
    double v = frame_lp(row, n_class, lane);
    if (r) v = ((double)(P - r) * v + (double)r * frame_lp(row + ld, n_class, lane)) / (double)P;
    acc += (double)g * v;
    gsum += g;
  }
  const bool on = lane < n_class;
  const double u = on ? (gsum > 0 ? acc / (double)gsum : 0.0) : -INFINITY;
  const double m = wave_max_d(u);
  const double d = on ? u - m : 0.0;
  const double sum = wave_sum_d(on ? exp(d) : 0.0);
  if (on) line_lp[((size_t)frame0 + j) * n_class + lane] = (float)(d - log(sum));
}

// grid (B), 256 threads.  line_lp rows (sum L, n_class); cls / start / end are arrays of sum L entries, a line's at its first row:
// the kept classes, then per kept symbol the first and the last line frame (0 .. L - 1) of its arg-max run; zero behind the length.
// Thread i takes the frames i * per .. of its line; the kept symbols and the run ends before it come from one block scan (the two
// counts share a word: at most 3201 each).
__global__ __launch_bounds__(256) void k_line_greedy(const float* __restrict__ line_lp, int n_class, const int* __restrict__ lines,
                                                      int max_L, int* __restrict__ cls, int* __restrict__ start, int* __restrict__ end,
                                                      int* __restrict__ len) {
  __shared__ unsigned char best[LR_MAX_L + 3];
  __shared__ unsigned wave_total[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frame0 = lines[2 * b], L = min(max(lines[2 * b + 1], 0), min(max_L, LR_MAX_L));
  for (int j = tid; j < L; j += 256) {
    const float* row = line_lp + ((size_t)frame0 + j) * n_class;
    float m = row[0];
    int arg = 0;
    for (int c = 1; c < n_class; ++c) {
      const float v = row[c];
      if (v > m) {                                                 // the first maximum
        m = v;
        arg = c;
      }
    }
    best[j] = (unsigned char)arg;
  }
  __syncthreads();
  const int per = (L + 255) / 256, lo = min(tid * per, L), hi = min(lo + per, L);
  unsigned cnt = 0;                                                // low half: runs that start in lo .. hi - 1, high half: runs that end there
  for (int j = lo; j < hi; ++j) {
    const int c = best[j];
    if (c == 0) continue;
    if (j == 0 || best[j - 1] != c) cnt += 1u;
    if (j == L - 1 || best[j + 1] != c) cnt += 1u << 16;
  }
  unsigned inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned below = __shfl_up(inc, o, 64);
    if (lane >= o) inc += below;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  unsigned before = inc - cnt, total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wave_total[w];
    total += wave_total[w];
  }
  int ks = (int)(before & 0xffffu), ke = (int)(before >> 16);
  const int n = (int)(total & 0xffffu);
  int* c_out = cls + frame0;
  int* s_out = start + frame0;
  int* e_out = end + frame0;
  for (int j = lo; j < hi; ++j) {
    const int c = best[j];
    if (c == 0) continue;
    if (j == 0 || best[j - 1] != c) {
      c_out[ks] = c;
      s_out[ks++] = j;
    }
    if (j == L - 1 || best[j + 1] != c) e_out[ke++] = j;
  }
  for (int i = n + tid; i < L; i += 256) c_out[i] = s_out[i] = e_out[i] = 0;
  if (tid == 0) len[b] = n;
}

// grid (B), 64 .. 1024 threads with K * blockDim.x >= 2 * max_L + 1.  Thread i holds the states i, i + blockDim.x, ..: state s is the
// blank for even s and symbol (s - 1) / 2 for odd s; a skip over the blank only between different labels.  alpha lives in LDS twice
// over (one barrier per frame); a thread's labels stay in registers and the log-probability of the next frame is loaded a frame ahead.
template <int K>
__global__ __launch_bounds__(1024) void k_line_ctc(const float* __restrict__ line_lp, int n_class, const int* __restrict__ lines,
                                                    int max_L, const int* __restrict__ cls, const int* __restrict__ len,
                                                    float* __restrict__ out) {
  __shared__ float alpha[2][LR_MAX_S + 1];
  __shared__ unsigned char lab[LR_MAX_L + 3];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int frame0 = lines[2 * b], L = min(max(lines[2 * b + 1], 1), min(max_L, LR_MAX_L));
  const int n = min(max(len[b], 0), L), S = 2 * n + 1;             // S <= 2 max_L + 1 <= K nt
  for (int i = tid; i < n; i += nt) lab[i] = (unsigned char)min(max(cls[frame0 + i], 0), n_class - 1);   // (a bad class stays inside the row)
  __syncthreads();
  const float* row = line_lp + (size_t)frame0 * n_class;
  int label[K];
  bool skip[K];
  float lp_next[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = tid + k * nt;
    const bool sym = s < S && (s & 1);
    label[k] = sym ? lab[s >> 1] : 0;
    skip[k] = sym && s >= 3 && label[k] != lab[(s >> 1) - 1];
    if (s < S) alpha[0][s] = s <= 1 ? row[label[k]] : -INFINITY;
    lp_next[k] = s < S && L > 1 ? row[n_class + label[k]] : 0.0f;
  }
  __syncthreads();
  for (int t = 1; t < L; ++t) {
    const float* prev = alpha[(t & 1) ^ 1];
    float* cur = alpha[t & 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int s = tid + k * nt;
      if (s < S) {
        const float lp = lp_next[k];
        if (t + 1 < L) lp_next[k] = row[(size_t)(t + 1) * n_class + label[k]];
        cur[s] = lse3(prev[s], s >= 1 ? prev[s - 1] : -INFINITY, skip[k] ? prev[s - 2] : -INFINITY) + lp;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* fin = alpha[(L - 1) & 1];
    out[b] = lse3(fin[S - 1], S > 1 ? fin[S - 2] : -INFINITY, -INFINITY);
  }
}

}  // namespace

extern "C" {

int dpmn_line_stitch_f32(const float* logits, int ld, int n_class, int T, int lr_w, const int* lines, const int* wins, const int* x0,
                         int B, int max_L, float* line_lp, dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && lines && wins && x0 && line_lp && B > 0 && B <= 65535 && T >= 2 && n_class > 0 && ld >= n_class && lr_w >= 2 &&
               lr_w <= LR_MAX_W && max_L > 0, "line_stitch: bad arguments");
  DPMN_REQUIRE(T <= LR_MAX_T && n_class <= LR_MAX_C && max_L <= LR_MAX_L,
               "line_stitch: at most 64 frames per window, 64 classes and 3201 frames per line");
  hipLaunchKernelGGL(k_line_stitch, dim3((unsigned)cdiv(max_L, 4), (unsigned)B), dim3(256), 0, as_stream(stream), logits, ld, n_class, T,
                     lr_w, lines, wins, x0, line_lp);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_line_greedy_i32(const float* line_lp, int n_class, const int* lines, int B, int max_L, int* cls, int* start, int* end,
                         int* length, dpmn_stream_t stream) {
  DPMN_REQUIRE(line_lp && lines && cls && start && end && length && B > 0 && n_class > 0 && max_L > 0, "line_greedy: bad arguments");
  DPMN_REQUIRE(n_class <= LR_MAX_C && max_L <= LR_MAX_L, "line_greedy: at most 64 classes and 3201 frames per line");
  hipLaunchKernelGGL(k_line_greedy, dim3((unsigned)B), dim3(256), 0, as_stream(stream), line_lp, n_class, lines, max_L, cls, start, end,
                     length);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_line_ctc_f32(const float* line_lp, int n_class, const int* lines, const int* cls, const int* length, float* out_score, int B,
                      int max_L, dpmn_stream_t stream) {
  DPMN_REQUIRE(line_lp && lines && cls && length && out_score && B > 0 && n_class > 0 && max_L > 0, "line_ctc: bad arguments");
  DPMN_REQUIRE(n_class <= LR_MAX_C && max_L <= LR_MAX_L, "line_ctc: at most 64 classes and 3201 frames per line");
  // the block: a thread per state up to 1024, then 2, 4 or 7 states per thread
  const int states = 2 * max_L + 1;
  const int threads = min(1024, cdiv(states, 64) * 64), per = cdiv(states, threads);
  static_assert(LR_MAX_K * 1024 >= LR_MAX_S, "line_ctc: the largest block must hold every state");
  const dim3 grid((unsigned)B), block((unsigned)threads);
  if (per <= 1)
    hipLaunchKernelGGL(k_line_ctc<1>, grid, block, 0, as_stream(stream), line_lp, n_class, lines, max_L, cls, length, out_score);
  else if (per <= 2)
    hipLaunchKernelGGL(k_line_ctc<2>, grid, block, 0, as_stream(stream), line_lp, n_class, lines, max_L, cls, length, out_score);
  else if (per <= 4)
    hipLaunchKernelGGL(k_line_ctc<4>, grid, block, 0, as_stream(stream), line_lp, n_class, lines, max_L, cls, length, out_score);
  else
    hipLaunchKernelGGL(k_line_ctc<LR_MAX_K>, grid, block, 0, as_stream(stream), line_lp, n_class, lines, max_L, cls, length, out_score);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
