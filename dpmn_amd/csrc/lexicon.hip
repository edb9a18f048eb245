// Lexicon-constrained reading (ours; main.py --rec_lexicon, utils/lexicon.py is the NumPy restatement).  A word is a 32-byte record:
// byte 0 its length n (1 .. 31), bytes 1 .. n its classes (1-based, 0 = the CTC blank), the rest 0.
//   k_ctc_lexicon   per (image, word) the CTC log-likelihood of the word under the image's frame posteriors (the forward / alpha
//                   recursion over the 2n + 1 states, fp32 in the log domain), per (image, slab of words) the best word
//   k_edit_lexicon  per (string, word) the Levenshtein distance (Hyyro's bit-parallel form of the DP: the string's <= 31 rows are
//                   the bits of one dword; integers only, exact), per (string, slab of words) the nearest word
//   k_lexicon_best  the slabs' partials of an image -> its best word.  "Best" is a total order (score, then the lower index), so
//                   the result does not depend on the order in which slabs, waves and lanes are combined.
// Neither kernel has a matrix product or a variant per compute mode.
#include "common.h"

namespace {

constexpr int LEX_REC = 32;          // bytes per word record
constexpr int LEX_MAX_T = 64;        // frames
constexpr int LEX_MAX_C = 64;        // classes (lane = class in the softmax)
constexpr int LEX_LD = LEX_MAX_C + 1;
constexpr int CTC_SLAB = 128;        // words per block: 4 waves x 32 words behind one log-softmax of the image
constexpr int EDIT_SLAB = 256;       // words per block: one per thread
constexpr int LEX_MAX_WORDS = 1 << 20;

// v of lane - 1 (wave_shr:1 crosses the rows of 16); lane 0 keeps `first`
__device__ __forceinline__ float lane_below(float first, float v) {
  return __uint_as_float(dpp_mov_u<0x138, 0xF>(__float_as_uint(first), __float_as_uint(v)));
}

// log(e^a + e^b + e^c); -inf when all three are
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
  v = min(v, xshfl<32>(v)); v = min(v, xshfl<16>(v)); v = min(v, xshfl<8>(v));
  v = min(v, xshfl<4>(v)); v = min(v, xshfl<2>(v)); v = min(v, xshfl<1>(v));
  return v;
}

// (score, index) a better than b: the higher score, the lower index among equals
__device__ __forceinline__ bool ctc_better(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// grid (slabs, B), 256 threads.  logits: rows b*T + t, leading dimension ld, columns >= n_class never read.  part: (B, slabs) pairs
// (score bits, index); a slab without a feasible word writes (-inf, -1).
// Phase 1: the image's log-softmax into LDS, one wave per frame, lane = class.  Phase 2: a wave walks its words one after the
// other, lane = CTC state s (label = blank for even s, symbol (s - 1) / 2 for odd s); the two lower neighbours' alphas come by DPP
// (no LDS round trip, no barrier inside the T loop), the emission is one LDS read.  Lanes >= 2n + 1 run along: a state only feeds
// higher states, so they never reach a live one.
__global__ __launch_bounds__(256) void k_ctc_lexicon(const float* __restrict__ logits, int ld, int n_class,
                                                      const unsigned char* __restrict__ words, int L, float* __restrict__ part, int T) {
  __shared__ float lp[LEX_MAX_T * LEX_LD];
  __shared__ float ws_[4];
  __shared__ int wi_[4];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = wave; t < T; t += 4) {
    const float x = lane < n_class ? logits[((size_t)b * T + t) * ld + lane] : -INFINITY;
    const float m = wave_max(x);
    const float sum = wave_sum(lane < n_class ? __expf(x - m) : 0.0f);
    lp[t * LEX_LD + lane] = x - m - __logf(sum);              // (lanes >= n_class: -inf, never read: a label is < n_class)
  }
  __syncthreads();
  const int w0 = slab * CTC_SLAB, w1 = min(w0 + CTC_SLAB, L);
  const int sym = lane >> 1;                                    // odd lane s: symbol (s - 1) / 2 = byte 1 + sym; its lower label: byte sym
  float best = -INFINITY;
  int best_i = -1;
  for (int w = w0 + wave; w < w1; w += 4) {
    const unsigned char* rec = words + (size_t)w * LEX_REC;
    const int n = min(__builtin_amdgcn_readfirstlane((int)rec[0]), LEX_REC - 1);
    if (n == 0) continue;                                       // (not a word; wave-uniform)
    int label = 0;
    bool skip = false;
    if ((lane & 1) && sym < n) {
      label = rec[1 + sym];
      skip = sym >= 1 && label != (int)rec[sym];
    }
    label = min(label, n_class - 1);                            // (a record is trusted to hold classes; a bad byte stays inside the row)
    float a = lane == 0 ? lp[0] : (lane == 1 ? lp[label] : -INFINITY);
    for (int t = 1; t < T; ++t) {
      const float e = lp[t * LEX_LD + label];
      const float p1 = lane_below(-INFINITY, a);
      const float p2 = lane_below(-INFINITY, p1);
      a = lse3(a, p1, skip ? p2 : -INFINITY) + e;
    }
    const float last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 2 * n));
    const float prev = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 2 * n - 1));
    const float s = lse3(last, prev, -INFINITY);
    if (s > best) { best = s; best_i = w; }                     // (words ascend: the first of equals stays)
  }
  if (lane == 0) { ws_[wave] = best; wi_[wave] = best_i; }
  __syncthreads();
  if (tid == 0) {
    float s = ws_[0];
    int i = wi_[0];
    for (int q = 1; q < 4; ++q)
      if (wi_[q] >= 0 && (i < 0 || ctc_better(ws_[q], wi_[q], s, i))) { s = ws_[q]; i = wi_[q]; }
    float* o = part + ((size_t)b * gridDim.x + slab) * 2;
    o[0] = s;
    o[1] = __int_as_float(i);
  }
}

// one wave per image: part (B, slabs) pairs -> best_idx[b], best_logp[b]
__global__ __launch_bounds__(64) void k_ctc_lexicon_best(const float* __restrict__ part, int slabs, int* __restrict__ best_idx,
                                                          float* __restrict__ best_logp) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float s = -INFINITY;
  int i = -1;
  for (int k = lane; k < slabs; k += 64) {
    const float* p = part + ((size_t)b * slabs + k) * 2;
    const float sk = p[0];
    const int ik = __float_as_int(p[1]);
    if (ik >= 0 && (i < 0 || ctc_better(sk, ik, s, i))) { s = sk; i = ik; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float so = xshfl_v(s, o);
    const int io = xshfl_v(i, o);
    if (io >= 0 && (i < 0 || ctc_better(so, io, s, i))) { s = so; i = io; }
  }
  if (lane == 0) { best_idx[b] = i; best_logp[b] = i < 0 ? -INFINITY : s; }
}

// Levenshtein distance between a string of m <= 31 symbols, given as its match masks peq[class] (bit i: symbol i is that class),
// and the word of record r (8 dwords): Hyyro 2003, the global-distance form of Myers' bit-vector DP.  The vertical deltas of a
// DP column are the bits of vp / vn; the column of word symbol j follows from the one before in a dozen integer operations.
__device__ __forceinline__ int edit_distance(const unsigned* __restrict__ peq, int m, const unsigned (&r)[8]) {
  const int n = r[0] & 0xff;
  if (m == 0) return n;
  const unsigned top = 1u << (m - 1);
  unsigned vp = ~0u, vn = 0u;
  int dist = m;
#pragma unroll
  for (int j = 1; j < LEX_REC; ++j) {
    if (j <= n) {
      const unsigned x = peq[(r[j >> 2] >> (8 * (j & 3))) & 0xff];
      const unsigned d0 = (((x & vp) + vp) ^ vp) | x | vn;
      unsigned hp = vn | ~(d0 | vp);
      unsigned hn = d0 & vp;
      dist += (hp & top) ? 1 : 0;
      dist -= (hn & top) ? 1 : 0;
      hp = (hp << 1) | 1u;
      hn <<= 1;
      vp = hn | ~(d0 | hp);
      vn = hp & d0;
    }
  }
  return dist;
}

// grid (slabs, B), 256 threads, one word per thread.  part (B, slabs): the least key (distance << 20 | word index) of the slab.
__global__ __launch_bounds__(256) void k_edit_lexicon(const unsigned char* __restrict__ strings, const unsigned char* __restrict__ words,
                                                       int L, unsigned* __restrict__ part) {
  __shared__ unsigned peq[256];
  __shared__ unsigned wk[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const unsigned char* str = strings + (size_t)b * LEX_REC;
  const int m = min((int)str[0], LEX_REC - 1);
  peq[tid] = 0u;
  __syncthreads();
  if (tid < m) atomicOr(&peq[str[1 + tid]], 1u << tid);
  __syncthreads();
  const int w = blockIdx.x * EDIT_SLAB + tid;
  unsigned key = ~0u;
  if (w < L) {
    const uint4* rp = reinterpret_cast<const uint4*>(words + (size_t)w * LEX_REC);
    const uint4 lo = rp[0], hi = rp[1];
    const unsigned r[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    key = ((unsigned)edit_distance(peq, m, r) << 20) | (unsigned)w;
  }
  key = wave_min_u(key);
  if ((tid & 63) == 0) wk[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = min(min(wk[0], wk[1]), min(wk[2], wk[3]));
}

// one wave per string: the least key of its slabs -> best_idx[b], best_dist[b]
__global__ __launch_bounds__(64) void k_edit_lexicon_best(const unsigned* __restrict__ part, int slabs, int* __restrict__ best_idx,
                                                           int* __restrict__ best_dist) {
  const int b = blockIdx.x, lane = threadIdx.x;
  unsigned key = ~0u;
  for (int k = lane; k < slabs; k += 64) key = min(key, part[(size_t)b * slabs + k]);
  key = wave_min_u(key);
  if (lane == 0) { best_idx[b] = (int)(key & (LEX_MAX_WORDS - 1)); best_dist[b] = (int)(key >> 20); }
}

}  // namespace

extern "C" {

size_t dpmn_ctc_lexicon_workspace_bytes(int B, int L) {
  return B > 0 && L > 0 ? (size_t)B * cdiv(L, CTC_SLAB) * 2 * sizeof(float) : 0;
}

int dpmn_ctc_lexicon_f32(const float* logits, int ld, int n_class, const unsigned char* words, int L, int* best_idx, float* best_logp,
                         void* ws, int B, int T, dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && words && best_idx && best_logp && ws && B > 0 && T > 0 && n_class > 0 && ld >= n_class, "ctc_lexicon: bad arguments");
  DPMN_REQUIRE(T <= LEX_MAX_T && n_class <= LEX_MAX_C, "ctc_lexicon: at most 64 frames and 64 classes");
  DPMN_REQUIRE(L > 0 && L <= LEX_MAX_WORDS && B <= 65535, "ctc_lexicon: 1 .. 2^20 words, at most 65535 images");
  DPMN_REQUIRE(((uintptr_t)ws & 3) == 0, "ctc_lexicon: the workspace must be 4-byte aligned");
  const int slabs = cdiv(L, CTC_SLAB);
  hipLaunchKernelGGL(k_ctc_lexicon, dim3((unsigned)slabs, (unsigned)B), dim3(256), 0, as_stream(stream), logits, ld, n_class, words, L,
                     (float*)ws, T);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ctc_lexicon_best, dim3((unsigned)B), dim3(64), 0, as_stream(stream), (const float*)ws, slabs, best_idx, best_logp);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

size_t dpmn_edit_lexicon_workspace_bytes(int B, int L) {
  return B > 0 && L > 0 ? (size_t)B * cdiv(L, EDIT_SLAB) * sizeof(unsigned) : 0;
}

int dpmn_edit_lexicon_i32(const unsigned char* strings, const unsigned char* words, int L, int* best_idx, int* best_dist, void* ws, int B,
                          dpmn_stream_t stream) {
  DPMN_REQUIRE(strings && words && best_idx && best_dist && ws && B > 0, "edit_lexicon: bad arguments");
  DPMN_REQUIRE(L > 0 && L <= LEX_MAX_WORDS && B <= 65535, "edit_lexicon: 1 .. 2^20 words, at most 65535 strings");
  DPMN_REQUIRE(((uintptr_t)words & 15) == 0 && ((uintptr_t)ws & 3) == 0, "edit_lexicon: the records must be 16-byte aligned, the workspace 4-byte");
  const int slabs = cdiv(L, EDIT_SLAB);
  hipLaunchKernelGGL(k_edit_lexicon, dim3((unsigned)slabs, (unsigned)B), dim3(256), 0, as_stream(stream), strings, words, L, (unsigned*)ws);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_edit_lexicon_best, dim3((unsigned)B), dim3(64), 0, as_stream(stream), (const unsigned*)ws, slabs, best_idx, best_dist);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
