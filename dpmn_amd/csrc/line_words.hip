// A tiled text line read as lexicon words (ours; main.py --rec_lexicon with --demo_tile --demo_line_read; utils/line_words.py is the
// NumPy restatement and gives the definition): the one-pass token-passing Viterbi over "blank gap, word, blank gap, word, ..." on the
// lexicon's prefix trie.  Per trie node a symbol state and a blank-after state, each with the frame at which its word was entered;
// per line the gap state G and, per frame, E = the best word end (score, then the lower word index: a total order, so the result does
// not depend on how lanes, waves and blocks are combined).  The float32 line posteriors widen exactly to fp64 and the recursion is
// fp64 + and compares only (the library is built with -ffp-contract=off): the bits of line_words_trie_np.
//   k_line_words_step  one launch per frame over (chunks of LW_BLOCK nodes, lines), the state double-buffered in global memory; block
//                      (0, line) first reduces the chunks' partials of the frame before into E[t-1], writes that frame's records and
//                      G[t].  A line shorter than the batch's longest stops at its own last frame.
//   k_line_words_lds   one launch per call, one block per line, both state buffers in LDS, one barrier per frame.
// Both write the same per-frame records (the word of E[t], its start, whether G[t] was entered from E[t-1]) and per line the fp64
// bits of G[L-1] and E[L-1]; utils.line_words.decode_records walks them on the host.  No kernel has a grid-wide barrier, a spin on a
// flag or a float atomic, a matrix product or a variant per compute mode.
#include "common.h"
#include <limits.h>

namespace {

constexpr int LW_MAX_L = 3201;               // frames per line (line_read.hip's limit)
constexpr int LW_MAX_C = 64;                 // classes
constexpr int LW_BLOCK = 256;                // k_line_words_step: nodes per block
constexpr int LW_MAX_NODES = 1 << 25;        // 2^20 words of 31 symbols stay below it
constexpr int LW_LDS_THREADS = 1024;         // k_line_words_lds: the largest block
constexpr int LW_LDS_K = 4;                  // ... and the most nodes per thread
constexpr int LW_LDS_WAVES = LW_LDS_THREADS / 64;
constexpr int LW_LDS_NODE_BYTES = 2 * (2 * 8 + 2 * 2);                 // two buffers of (sym, blk) fp64 and their starts as u16
constexpr int LW_LDS_FIXED_BYTES = 2 * LW_LDS_WAVES * (8 + 4 + 4);     // two buffers of the waves' E candidates
constexpr int LW_NO_WORD = INT_MAX;

struct LwPart { double s; int w; int st; };  // a block's best word end of one frame: score, word, start

__device__ __forceinline__ bool lw_better(double sa, int wa, double sb, int wb) { return sa > sb || (sa == sb && wa < wb); }

__device__ __forceinline__ void lw_wave_best(double& s, int& w, int& st) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double so = xshfl_v(s, o);
    const int wo = xshfl_v(w, o), sto = xshfl_v(st, o);
    if (lw_better(so, wo, s, w)) { s = so; w = wo; st = sto; }
  }
}

// One node, one frame.  (a, sa) / (b, sb): its symbol / blank state of the frame before; (pb, spb) / (pa, spa): its parent's blank /
// symbol state (unused for a first symbol: there gpen = G[t-1] + pen enters with start t).  max3 / max2 keep the FIRST maximum.
__device__ __forceinline__ void lw_node(bool top, bool same, double a, int sa, double b, int sb, double pb, int spb, double pa, int spa,
                                        double gpen, int t, double lpc, double lp0, double& na, int& nsa, double& nb, int& nsb) {
  double best = a;
  int st = sa;
  if (top) {
    if (gpen > best) { best = gpen; st = t; }
  } else {
    if (pb > best) { best = pb; st = spb; }
    if (!same && pa > best) { best = pa; st = spa; }
  }
  na = lpc + best;
  nsa = st;
  if (a > b) { nb = lp0 + a; nsb = sa; } else { nb = lp0 + b; nsb = sb; }
}

struct LwState { double* sym; double* blk; int* s_sym; int* s_blk; };

// the state of (line b, parity q): 24 N bytes, the doubles first
__device__ __forceinline__ LwState lw_state(unsigned char* state, int b, int q, int N) {
  LwState s;
  s.sym = reinterpret_cast<double*>(state + ((size_t)b * 2 + q) * 24 * (size_t)N);
  s.blk = s.sym + N;
  s.s_sym = reinterpret_cast<int*>(s.blk + N);
  s.s_blk = s.s_sym + N;
  return s;
}

// grid (chunks, B), LW_BLOCK threads, launched for t = 0 .. max_L.  line_lp rows (sum L, ld), columns >= n_class never read.  G: one
// double per line frame.  part (B, 2, chunks).  rec_w / rec_s / rec_g: one int per line frame; fin (B, 4): the bits of G[L-1], E[L-1].
__global__ __launch_bounds__(LW_BLOCK) void k_line_words_step(const float* __restrict__ line_lp, int ld, int n_class,
                                                               const int* __restrict__ lines, const int4* __restrict__ trie, int N,
                                                               int chunks, double pen, int t, double* __restrict__ G,
                                                               LwPart* __restrict__ part, unsigned char* __restrict__ state,
                                                               int* __restrict__ rec_w, int* __restrict__ rec_s, int* __restrict__ rec_g,
                                                               int* __restrict__ fin) {
  __shared__ double sh_s[LW_BLOCK / 64];
  __shared__ int sh_w[LW_BLOCK / 64], sh_st[LW_BLOCK / 64];
  __shared__ float row[LW_MAX_C];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = lines[2 * b], L = min(lines[2 * b + 1], LW_MAX_L);
  if (t > L) return;                                               // (uniform over the block: the line ended before this launch)
  LwPart* mine = part + (size_t)b * 2 * chunks;
  if (chunk == 0 && t == 0 && tid == 0) {
    G[f0] = (double)line_lp[(size_t)f0 * ld];
    rec_g[f0] = 0;
  }
  if (chunk == 0 && t >= 1) {
    // E[t-1]: the best of the chunks' partials of the frame before
    const LwPart* p = mine + (size_t)((t - 1) & 1) * chunks;
    double s = -INFINITY;
    int w = LW_NO_WORD, st = 0;
    for (int k = tid; k < chunks; k += LW_BLOCK) {
      const LwPart c = p[k];
      if (lw_better(c.s, c.w, s, w)) { s = c.s; w = c.w; st = c.st; }
    }
    lw_wave_best(s, w, st);
    if (lane == 0) { sh_s[wave] = s; sh_w[wave] = w; sh_st[wave] = st; }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < LW_BLOCK / 64; ++q)
        if (lw_better(sh_s[q], sh_w[q], s, w)) { s = sh_s[q]; w = sh_w[q]; st = sh_st[q]; }
      rec_w[f0 + t - 1] = w == LW_NO_WORD ? 0 : w;
      rec_s[f0 + t - 1] = st;
      const double g = G[f0 + t - 1];
      if (t == L) {
        fin[4 * b] = __double2loint(g);
        fin[4 * b + 1] = __double2hiint(g);
        fin[4 * b + 2] = __double2loint(s);
        fin[4 * b + 3] = __double2hiint(s);
      } else {
        const bool enter = s > g;                                  // (a tie stays in G)
        G[f0 + t] = (double)line_lp[(size_t)(f0 + t) * ld] + (enter ? s : g);
        rec_g[f0 + t] = enter ? 1 : 0;
      }
    }
  }
  if (t == L) return;                                              // (uniform)
  if (tid < n_class) row[tid] = line_lp[(size_t)(f0 + t) * ld + tid];
  __syncthreads();                                                 // (also: thread 0 is done with sh_* of the head)
  const int v = chunk * LW_BLOCK + tid;
  double cs = -INFINITY;
  int cw = LW_NO_WORD, cst = 0;
  if (v < N) {
    const int4 nd = trie[v];                                       // parent, class, same as the parent's class, word
    const int c = min(max(nd.y, 0), n_class - 1);                  // (a bad class stays inside the row)
    const bool top = nd.x < 0;
    const LwState cur = lw_state(state, b, t & 1, N);
    double na, nb;
    int nsa, nsb;
    if (t == 0) {
      na = top ? (double)row[c] + pen : -INFINITY;
      nb = -INFINITY;
      nsa = nsb = 0;
    } else {
      const LwState prev = lw_state(state, b, (t - 1) & 1, N);
      const int p = top ? 0 : min(nd.x, N - 1);
      lw_node(top, nd.z != 0, prev.sym[v], prev.s_sym[v], prev.blk[v], prev.s_blk[v], prev.blk[p], prev.s_blk[p], prev.sym[p], prev.s_sym[p],
              G[f0 + t - 1] + pen, t, (double)row[c], (double)row[0], na, nsa, nb, nsb);
    }
    cur.sym[v] = na;
    cur.blk[v] = nb;
    cur.s_sym[v] = nsa;
    cur.s_blk[v] = nsb;
    if (nd.w >= 0) { cs = na; cw = nd.w; cst = nsa; }
  }
  lw_wave_best(cs, cw, cst);
  if (lane == 0) { sh_s[wave] = cs; sh_w[wave] = cw; sh_st[wave] = cst; }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < LW_BLOCK / 64; ++q)
      if (lw_better(sh_s[q], sh_w[q], cs, cw)) { cs = sh_s[q]; cw = sh_w[q]; cst = sh_st[q]; }
    LwPart o;
    o.s = cs; o.w = cw; o.st = cst;
    mine[(size_t)(t & 1) * chunks + chunk] = o;
  }
}

// grid (B), 64 .. 1024 threads with K * blockDim.x >= N.  Thread i holds the nodes i, i + blockDim.x, ..: the trie entries and the
// nodes' own states stay in registers, LDS holds both buffers of every node's state for the children to read (starts as u16: a
// frame is < 3201) and both buffers of the waves' E candidates.  Every thread follows G and E itself; thread 0 writes the records.
template <int K>
__global__ __launch_bounds__(LW_LDS_THREADS) void k_line_words_lds(const float* __restrict__ line_lp, int ld, int n_class,
                                                                    const int* __restrict__ lines, const int4* __restrict__ trie, int N,
                                                                    double pen, int* __restrict__ rec_w, int* __restrict__ rec_s,
                                                                    int* __restrict__ rec_g, int* __restrict__ fin) {
  extern __shared__ double lw_smem[];
  double* sym = lw_smem;                                           // [2][N]
  double* blk = sym + 2 * (size_t)N;                               // [2][N]
  double* wp_s = blk + 2 * (size_t)N;                              // [2][LW_LDS_WAVES]
  int* wp_w = reinterpret_cast<int*>(wp_s + 2 * LW_LDS_WAVES);     // [2][LW_LDS_WAVES]
  int* wp_st = wp_w + 2 * LW_LDS_WAVES;
  unsigned short* s_sym = reinterpret_cast<unsigned short*>(wp_st + 2 * LW_LDS_WAVES);   // [2][N]
  unsigned short* s_blk = s_sym + 2 * (size_t)N;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = nt >> 6;
  const int f0 = lines[2 * b], L = min(max(lines[2 * b + 1], 1), LW_MAX_L);
  const float* lp = line_lp + (size_t)f0 * ld;
  int parent[K], cls[K], word[K], sa[K], sb[K];
  bool top[K], same[K];
  double a[K], bl[K];
  float lp_next[K];
  double cs = -INFINITY;
  int cw = LW_NO_WORD, cst = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int v = tid + k * nt;
    const int4 nd = v < N ? trie[v] : make_int4(-1, 0, 0, -1);
    top[k] = nd.x < 0;
    parent[k] = top[k] ? 0 : min(nd.x, N - 1);
    cls[k] = min(max(nd.y, 0), n_class - 1);
    same[k] = nd.z != 0;
    word[k] = nd.w;
    a[k] = top[k] ? (double)lp[cls[k]] + pen : -INFINITY;
    bl[k] = -INFINITY;
    sa[k] = sb[k] = 0;
    lp_next[k] = L > 1 ? lp[ld + cls[k]] : 0.0f;
    if (v < N) {
      sym[v] = a[k];
      blk[v] = bl[k];
      s_sym[v] = s_blk[v] = 0;
      if (word[k] >= 0 && lw_better(a[k], word[k], cs, cw)) { cs = a[k]; cw = word[k]; cst = 0; }
    }
  }
  lw_wave_best(cs, cw, cst);
  if (lane == 0) { wp_s[wave] = cs; wp_w[wave] = cw; wp_st[wave] = cst; }
  double g = (double)lp[0];
  float lp0_next = L > 1 ? lp[ld] : 0.0f;
  if (tid == 0) rec_g[f0] = 0;
  __syncthreads();
  for (int t = 1; t <= L; ++t) {
    const int q = t & 1, qp = q ^ 1;
    // E[t-1]: the best of the waves' candidates of the frame before
    double es = wp_s[qp * LW_LDS_WAVES];
    int ew = wp_w[qp * LW_LDS_WAVES], est = wp_st[qp * LW_LDS_WAVES];
    for (int i = 1; i < waves; ++i) {
      const double s = wp_s[qp * LW_LDS_WAVES + i];
      const int w = wp_w[qp * LW_LDS_WAVES + i];
      if (lw_better(s, w, es, ew)) { es = s; ew = w; est = wp_st[qp * LW_LDS_WAVES + i]; }
    }
    if (tid == 0) {
      rec_w[f0 + t - 1] = ew == LW_NO_WORD ? 0 : ew;
      rec_s[f0 + t - 1] = est;
    }
    if (t == L) {
      if (tid == 0) {
        fin[4 * b] = __double2loint(g);
        fin[4 * b + 1] = __double2hiint(g);
        fin[4 * b + 2] = __double2loint(es);
        fin[4 * b + 3] = __double2hiint(es);
      }
      break;
    }
    const bool enter = es > g;                                     // (a tie stays in G)
    const double gpen = g + pen, lp0 = (double)lp0_next;
    g = lp0 + (enter ? es : g);
    if (tid == 0) rec_g[f0 + t] = enter ? 1 : 0;
    if (t + 1 < L) lp0_next = lp[(size_t)(t + 1) * ld];
    const double* psym = sym + (size_t)qp * N;
    const double* pblk = blk + (size_t)qp * N;
    const unsigned short* ps_sym = s_sym + (size_t)qp * N;
    const unsigned short* ps_blk = s_blk + (size_t)qp * N;
    cs = -INFINITY;
    cw = LW_NO_WORD;
    cst = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int v = tid + k * nt;
      if (v < N) {
        const double lpc = (double)lp_next[k];
        if (t + 1 < L) lp_next[k] = lp[(size_t)(t + 1) * ld + cls[k]];
        const int p = parent[k];
        double na, nb;
        int nsa, nsb;
        lw_node(top[k], same[k], a[k], sa[k], bl[k], sb[k], pblk[p], (int)ps_blk[p], psym[p], (int)ps_sym[p], gpen, t, lpc, lp0, na, nsa,
                nb, nsb);
        a[k] = na; bl[k] = nb; sa[k] = nsa; sb[k] = nsb;
        sym[(size_t)q * N + v] = na;
        blk[(size_t)q * N + v] = nb;
        s_sym[(size_t)q * N + v] = (unsigned short)nsa;
        s_blk[(size_t)q * N + v] = (unsigned short)nsb;
        if (word[k] >= 0 && lw_better(na, word[k], cs, cw)) { cs = na; cw = word[k]; cst = nsa; }
      }
    }
    lw_wave_best(cs, cw, cst);
    if (lane == 0) { wp_s[q * LW_LDS_WAVES + wave] = cs; wp_w[q * LW_LDS_WAVES + wave] = cw; wp_st[q * LW_LDS_WAVES + wave] = cst; }
    __syncthreads();
  }
}

size_t lw_lds_bytes(int N) { return (size_t)N * LW_LDS_NODE_BYTES + LW_LDS_FIXED_BYTES; }

}  // namespace

extern "C" {

int dpmn_line_words_block(void) { return LW_BLOCK; }

int dpmn_line_words_lds_nodes(void) {
  const long by_lds = ((long)dpmn_lds_limit() - LW_LDS_FIXED_BYTES) / LW_LDS_NODE_BYTES;
  return (int)max(0L, min(by_lds, (long)LW_LDS_THREADS * LW_LDS_K));
}

size_t dpmn_line_words_workspace_bytes(int B, int frames, int nodes) {
  if (B <= 0 || frames <= 0 || nodes <= 0) return 0;
  const size_t chunks = (size_t)cdiv(nodes, LW_BLOCK);
  return (size_t)frames * sizeof(double) + (size_t)B * 2 * chunks * sizeof(LwPart) + (size_t)B * 2 * 24 * (size_t)nodes;
}

int dpmn_line_words_f64(const float* line_lp, int ld, int n_class, const int* lines, int B, int max_L, int frames, const int* trie,
                        int nodes, double penalty, int arm, int* rec_word, int* rec_start, int* rec_enter, int* fin, void* ws,
                        dpmn_stream_t stream) {
  DPMN_REQUIRE(line_lp && lines && trie && rec_word && rec_start && rec_enter && fin && B > 0 && B <= 65535 && n_class > 0 &&
               ld >= n_class && max_L > 0 && frames >= max_L && nodes > 0 && (arm == 0 || arm == 1), "line_words: bad arguments");
  DPMN_REQUIRE(n_class <= LW_MAX_C && max_L <= LW_MAX_L, "line_words: at most 64 classes and 3201 frames per line");
  DPMN_REQUIRE(nodes <= LW_MAX_NODES, "line_words: at most 2^25 trie nodes");
  DPMN_REQUIRE(penalty - penalty == 0.0, "line_words: the penalty must be finite");
  DPMN_REQUIRE(((uintptr_t)trie & 15) == 0, "line_words: the trie must be 16-byte aligned");
  const double pen = 0.0 + penalty;
  const int4* nodes4 = reinterpret_cast<const int4*>(trie);
  if (arm == 1) {
    DPMN_REQUIRE(nodes <= dpmn_line_words_lds_nodes(), "line_words: the trie does not fit the single-launch arm's LDS");
    const int threads = min(LW_LDS_THREADS, cdiv(nodes, 64) * 64), per = cdiv(nodes, threads);
    const size_t smem = lw_lds_bytes(nodes);
    const dim3 grid((unsigned)B), block((unsigned)threads);
#define LW_LDS_LAUNCH(K_)                                                                                                             \
  do {                                                                                                                                \
    dpmn_lds_optin<k_line_words_lds<K_>>(smem);                                                                                       \
    hipLaunchKernelGGL(k_line_words_lds<K_>, grid, block, smem, as_stream(stream), line_lp, ld, n_class, lines, nodes4, nodes, pen,   \
                       rec_word, rec_start, rec_enter, fin);                                                                          \
  } while (0)
    if (per <= 1) LW_LDS_LAUNCH(1);
    else if (per <= 2) LW_LDS_LAUNCH(2);
    else LW_LDS_LAUNCH(LW_LDS_K);
#undef LW_LDS_LAUNCH
    DPMN_CHECK_LAUNCH();
    return DPMN_OK;
  }
  DPMN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "line_words: the workspace must be 8-byte aligned");
  const int chunks = cdiv(nodes, LW_BLOCK);
  double* G = reinterpret_cast<double*>(ws);
  LwPart* part = reinterpret_cast<LwPart*>(G + frames);
  unsigned char* state = reinterpret_cast<unsigned char*>(part + (size_t)B * 2 * chunks);
  for (int t = 0; t <= max_L; ++t) {
    hipLaunchKernelGGL(k_line_words_step, dim3((unsigned)chunks, (unsigned)B), dim3(LW_BLOCK), 0, as_stream(stream), line_lp, ld, n_class,
                       lines, nodes4, nodes, chunks, pen, t, G, part, state, rec_word, rec_start, rec_enter, fin);
    DPMN_CHECK_LAUNCH();
  }
  return DPMN_OK;
}

}  // extern "C"
