// CTC prefix beam search with a character n-gram model (ours; main.py --rec_beam / --rec_lm, utils/beam.py is the definition and the
// NumPy restatement; Hannun et al. 2014).
//   k_ctc_beam   one launch per batch, ONE WAVE per image: the image's log-softmax in fp64 into LDS, then T frames of
//                "offer, pick the `width` best, rebuild the beam", everything in LDS.  A member of the beam is pb, pnb, lm (fp64), its
//                last class, its context index in the model's table and its own symbols (a byte each, 64 bytes, zero behind the
//                end).  Prefix identity is EXACT: member j is the extension of member i by class c iff len(j) == len(i) + 1,
//                last(j) == c and the symbols of j without the last equal those of i, compared word by word in LDS -- no node ids,
//                which a dropped and recreated prefix would get twice while its descendants still sit in the beam.
//                The candidates of a frame are the slots i * n_class + c (c == 0: member i itself; c > 0: its extension by c), at
//                most 32 * 64; the slot number is also the tie order (parent rank, then class).  The `width` best are taken by
//                `width` rounds of a wave-wide arg-max over the slots' rank scores in LDS.
// One wave and not four: the work of a frame is a few hundred fp64 additions, about 32 log-sum-exps and `width` dependent arg-max
// rounds; it is a latency chain, and with one wave every phase boundary is a wave-local barrier and the arg-max needs no LDS
// round trip between waves.  B = 48 images occupy 48 of the 256 CUs whatever the block size.
// All arithmetic on scores is fp64, in the order utils/beam.py writes it (the library is built with -ffp-contract=off).
// No call depends on the compute mode.
#include "common.h"

namespace {

constexpr int BM_MAX_T = 64;         // frames
constexpr int BM_MAX_C = 64;         // classes
constexpr int BM_MAX_W = 32;         // beam width
constexpr int BM_LM_C = 37;          // the model's classes (the CRNN's): row length of its table
constexpr int BM_WORDS = BM_MAX_T / 4;   // dwords of a member's symbols
constexpr int BM_SLOTS = BM_MAX_W * BM_MAX_C;

// log(e^a + e^b) = m + log(exp(a - m) + exp(b - m)); -inf when both are (utils.beam.lse)
__device__ __forceinline__ double lse2(double a, double b) {
  const double m = a > b ? a : b;
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m));
}

// (score, index) a before b: the higher score, the lower index among equals
__device__ __forceinline__ bool bm_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// the wave's first (score, index) in bm_before's order, in every lane
__device__ __forceinline__ void wave_first(double& s, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double so = xshfl_v(s, o);
    const int io = xshfl_v(i, o);
    if (bm_before(so, io, s, i)) { s = so; i = io; }
  }
}

// grid (B), 64 threads.  logits: rows b*T + t, leading dimension ld, columns >= n_class never read.  table: the model's float32 natural
// logs (n_ctx, 37), or null (then alpha is 0).  out_cls (B, T), out_len (B), out_score (B, 2): the bits of the fp64 score, low dword first.
__global__ __launch_bounds__(64) void k_ctc_beam(const float* __restrict__ logits, int ld, int n_class, const float* __restrict__ table,
                                                  int n_ctx, int width, double alpha, double beta, int* __restrict__ out_cls,
                                                  int* __restrict__ out_len, int* __restrict__ out_score, int T) {
  __shared__ double lp[BM_MAX_T * BM_MAX_C];          // row t at t * n_class
  __shared__ double score[BM_SLOTS];                  // a frame's rank scores by slot; -inf: no candidate, or taken
  __shared__ double pb[2][BM_MAX_W], pnb[2][BM_MAX_W], lm[2][BM_MAX_W];
  __shared__ double tot[BM_MAX_W], spb[BM_MAX_W], spnb[BM_MAX_W];
  __shared__ unsigned sym[2][BM_MAX_W][BM_WORDS];
  __shared__ int len[2][BM_MAX_W], last[2][BM_MAX_W], ctx[2][BM_MAX_W];
  __shared__ int par[BM_MAX_W];                       // the member whose extension by last[j] member j is, or -1
  __shared__ int win[BM_MAX_W];                       // the slots picked in a frame, best first
  __shared__ signed char child[BM_SLOTS];             // slot (i, c) -> the member that IS p_i + c, or -1
  const int b = blockIdx.x, lane = threadIdx.x;
  const int C = n_class;

  // the image's log-softmax: lane = class stages the row, lane = frame takes its log-sum-exp (classes in ascending order)
  if (lane < C)
    for (int t = 0; t < T; ++t) lp[t * C + lane] = (double)logits[((size_t)b * T + t) * ld + lane];
  __syncthreads();
  if (lane < T) {
    double* r = lp + lane * C;
    double m = r[0];
    for (int c = 1; c < C; ++c) m = r[c] > m ? r[c] : m;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += exp(r[c] - m);
    const double ls = log(sum);
    for (int c = 0; c < C; ++c) r[c] = (r[c] - m) - ls;
  }
  // the empty prefix
  if (lane < BM_MAX_W) {
    pb[0][lane] = lane == 0 ? 0.0 : -INFINITY;
    pnb[0][lane] = -INFINITY;
    lm[0][lane] = 0.0;
    len[0][lane] = 0; last[0][lane] = 0; ctx[0][lane] = 0;
  }
  for (int k = lane; k < BM_MAX_W * BM_WORDS; k += 64) sym[0][k / BM_WORDS][k % BM_WORDS] = 0u;
  __syncthreads();

  int n = 1;                                           // members (wave-uniform)
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const double* row = lp + t * C;
    const int slots = n * C;
    // phase 1: every member's total and its parent in the beam; the child table cleared
    if (lane < n) {
      tot[lane] = lse2(pb[cur][lane], pnb[cur][lane]);
      const int lj = len[cur][lane];
      int p = -1;
      for (int i = 0; i < n; ++i) {
        if (len[cur][i] + 1 != lj) continue;
        bool same = true;
        for (int w = 0; 4 * w < lj; ++w) {
          unsigned q = sym[cur][lane][w];
          if (w == (lj - 1) >> 2) q &= ~(0xffu << (8 * ((lj - 1) & 3)));      // member j without its last symbol
          same = same && q == sym[cur][i][w];
        }
        if (same) p = i;
      }
      par[lane] = p;
    }
    for (int s = lane; s < slots; s += 64) child[s] = -1;
    __syncthreads();
    if (lane < n && par[lane] >= 0) child[par[lane] * C + last[cur][lane]] = (signed char)lane;
    __syncthreads();
    // phase 2: the offers.  A member itself (slot i * C): blank after anything, its own symbol again, and the offer of its parent
    if (lane < n) {
      const int e = last[cur][lane], p = par[lane];
      const double own = len[cur][lane] > 0 ? pnb[cur][lane] + row[e] : -INFINITY;
      double ext = -INFINITY;
      if (p >= 0) ext = ((len[cur][p] > 0 && e == last[cur][p]) ? pb[cur][p] : tot[p]) + row[e];
      const double nb = tot[lane] + row[0], nnb = lse2(own, ext);
      spb[lane] = nb;
      spnb[lane] = nnb;
      score[lane * C] = lse2(nb, nnb) + lm[cur][lane];
    }
    for (int s = lane; s < slots; s += 64) {
      const int i = s / C, c = s - i * C;
      if (c == 0) continue;
      double v = -INFINITY;
      if (child[s] < 0) {
        const double a = ((len[cur][i] > 0 && c == last[cur][i]) ? pb[cur][i] : tot[i]) + row[c];
        const double l = table ? (double)table[(size_t)ctx[cur][i] * BM_LM_C + c] : 0.0;
        v = a + (lm[cur][i] + (alpha * l + beta));
      }
      score[s] = v;
    }
    __syncthreads();
    // phase 3: the `width` best slots, one wave-wide arg-max each; a slot that is picked leaves the table
    int n_new = 0;
    for (int r = 0; r < width; ++r) {
      double best = -INFINITY;
      int at = BM_SLOTS;
      for (int s = lane; s < slots; s += 64) {
        const double v = score[s];
        if (v > best) { best = v; at = s; }            // (slots ascend: the first of equals stays)
      }
      wave_first(best, at);
      if (best == -INFINITY) break;                    // (wave-uniform: every lane holds the same pair)
      if (lane == 0) { win[r] = at; score[at] = -INFINITY; }
      n_new = r + 1;
      __syncthreads();
    }
    __syncthreads();
    // phase 4: the next beam, in the order picked
    if (lane < n_new) {
      const int s = win[lane], i = s / C, c = s - i * C;
      if (c == 0) {
        pb[nxt][lane] = spb[i];
        pnb[nxt][lane] = spnb[i];
        lm[nxt][lane] = lm[cur][i];
        len[nxt][lane] = len[cur][i]; last[nxt][lane] = last[cur][i]; ctx[nxt][lane] = ctx[cur][i];
      } else {
        const double l = table ? (double)table[(size_t)ctx[cur][i] * BM_LM_C + c] : 0.0;
        pb[nxt][lane] = -INFINITY;
        pnb[nxt][lane] = ((len[cur][i] > 0 && c == last[cur][i]) ? pb[cur][i] : tot[i]) + row[c];
        lm[nxt][lane] = lm[cur][i] + (alpha * l + beta);
        len[nxt][lane] = len[cur][i] + 1; last[nxt][lane] = c; ctx[nxt][lane] = (ctx[cur][i] * BM_LM_C + c) % n_ctx;
      }
    }
    for (int k = lane; k < n_new * BM_WORDS; k += 64) {
      const int r = k / BM_WORDS, w = k - r * BM_WORDS;
      const int s = win[r], i = s / C, c = s - i * C;
      unsigned q = sym[cur][i][w];
      const int li = len[cur][i];                      // (li <= t <= 63: the new symbol's byte lies inside the 64)
      if (c > 0 && w == li >> 2) q |= (unsigned)c << (8 * (li & 3));
      sym[nxt][r][w] = q;
    }
    n = n_new;
    __syncthreads();
  }

  // the end of the word, then the best member (ties: the lower rank)
  const int fin = T & 1;
  double s = -INFINITY;
  int at = lane;
  if (lane < n) {
    const double l = table ? (double)table[(size_t)ctx[fin][lane] * BM_LM_C] : 0.0;
    s = lse2(pb[fin][lane], pnb[fin][lane]) + (lm[fin][lane] + alpha * l);
  }
  wave_first(s, at);
  if (at >= n) at = 0;                                 // (every score -inf: cannot happen with finite logits; stay inside the beam)
  const int L = min(len[fin][at], T);
  for (int k = lane; k < T; k += 64)
    out_cls[(size_t)b * T + k] = k < L ? (int)((sym[fin][at][k >> 2] >> (8 * (k & 3))) & 0xffu) : 0;
  if (lane == 0) {
    const long long bits = __double_as_longlong(s);
    out_len[b] = L;
    out_score[2 * b] = (int)(bits & 0xffffffffll);
    out_score[2 * b + 1] = (int)(bits >> 32);
  }
}

}  // namespace

extern "C" {

int dpmn_ctc_beam_f64(const float* logits, int ld, int n_class, const float* lm_table, int lm_order, int width, double alpha, double beta,
                      int* out_cls, int* out_len, int* out_score, int B, int T, dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && out_cls && out_len && out_score && B > 0 && T > 0 && n_class > 1 && ld >= n_class, "ctc_beam: bad arguments");
  DPMN_REQUIRE(T <= BM_MAX_T && n_class <= BM_MAX_C, "ctc_beam: at most 64 frames and 64 classes");
  DPMN_REQUIRE(width >= 1 && width <= BM_MAX_W, "ctc_beam: the width is 1 .. 32");
  DPMN_REQUIRE(alpha == alpha && beta == beta && alpha - alpha == 0.0 && beta - beta == 0.0, "ctc_beam: alpha and beta must be finite");
  DPMN_REQUIRE(lm_table ? (lm_order >= 1 && lm_order <= 3 && n_class <= BM_LM_C) : lm_order == 0,
               "ctc_beam: a model has order 1 .. 3 and at most 37 classes; without a model the order is 0");
  int n_ctx = 1;
  for (int k = 1; k < lm_order; ++k) n_ctx *= BM_LM_C;
  hipLaunchKernelGGL(k_ctc_beam, dim3((unsigned)B), dim3(64), 0, as_stream(stream), logits, ld, n_class, lm_table, n_ctx, width,
                     lm_table ? alpha : 0.0, beta, out_cls, out_len, out_score, T);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
