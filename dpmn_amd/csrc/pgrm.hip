// PGRM-specific kernels (everything that is not a plain GEMM) and the native forward driver.
//
// Token layout: (B, L, C) row-major fp32 with token t <-> (t / W, t % W) -- the reference's own
// layout (pgrm.py:423), i.e. NHWC over the 16x64 patch grid.  The window-attention output is
// written in WINDOW-MAJOR order without un-roll / window_reverse (quirk Q1, pgrm.py:263), which is
// exactly the contiguous order in which a per-window workgroup produces it.
//
// Reference lines: PatchEmbed 419-426 (+prior_fusion 548), WindowAttention.forward 197-266,
// SKConv gate 86-91, Mlp depthwise 34-36, tail 559-565, SwinTransformerBlock.forward 315-331,
// PGRM.forward 546-565.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------- patch embed
// One wave = 16 tokens; lane -> (token = l>>2, part = l&3).  Each lane produces C/4 embedding channels of its
// token; with the fused prior_fusion conv3x3 (2->3, pad 1) each lane first evaluates ONE of the 2x2 patch pixels
// and the four lanes of a token exchange results by shuffle.  pe weights sit in LDS transposed ([k][c]) so the
// four parts read distinct banks.  The finished rows leave through a wave-private LDS tile as contiguous 1 KB stores (end of the kernel).
template <int C, int PATCH, bool FUSE>
__global__ __launch_bounds__(256) void k_patch_embed_ln(const float* __restrict__ img, int cin, const float* __restrict__ pf_w,
                                                         const float* __restrict__ pf_b, const float* __restrict__ pe_w,
                                                         const float* __restrict__ pe_b, const float* __restrict__ ln_w,
                                                         const float* __restrict__ ln_b, float* __restrict__ tok, int B,
                                                         int Hi, int Wi, float p_drop, unsigned long long seed) {
  // p_drop > 0: pos_drop (pgrm.py:550-551) on the way out -- the mask of dpmn_dropout_f32(tokens, n = M C, p_drop, seed) applied to the
  // finished LayerNorm output (same product, bitwise), one launch and one pass over the tokens less per stream
  constexpr int CQ = C / 4, KP = 3 * PATCH * PATCH;
  static_assert(!FUSE || PATCH == 2, "fused prior conv assumes 2x2 patches (one pixel per lane of the token quad)");
  __shared__ __attribute__((aligned(16))) float wt[KP * C];
  __shared__ float pfw[3 * 2 * 9 + 3];
  constexpr int LDT = C + 4;
  __shared__ __attribute__((aligned(16))) float stg[4 * 16 * LDT];   // per wave: 16 finished token rows on their way out
  for (int i = threadIdx.x; i < KP * C; i += 256) wt[(i % KP) * C + i / KP] = pe_w[i];   // pe_w (C, KP) -> [k][c]
  if (FUSE && threadIdx.x < 57) pfw[threadIdx.x] = threadIdx.x < 54 ? pf_w[threadIdx.x] : pf_b[threadIdx.x - 54];
  __syncthreads();
  const int Ht = Hi / PATCH, Wt = Wi / PATCH;
  const int lane = threadIdx.x & 63;
  long token = (long)blockIdx.x * 64 + (threadIdx.x >> 6) * 16 + (lane >> 2);
  const long ntok = (long)B * Ht * Wt;
  const bool valid = token < ntok;
  if (!valid) token = ntok - 1;
  const int part = lane & 3;
  const int b = token / (Ht * Wt), t = token % (Ht * Wt);
  const int th = t / Wt, tw = t % Wt;
  float in[KP];
  if (FUSE) {
    const int dy = part >> 1, dx = part & 1;
    const int y = th * 2 + dy, x = tw * 2 + dx;
    float a[3] = {pfw[54], pfw[55], pfw[56]};
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = x + kx - 1;
          const bool inb = yy >= 0 && yy < Hi && xx >= 0 && xx < Wi;
          const float v = inb ? img[(((size_t)b * 2 + ci) * Hi + yy) * Wi + xx] : 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) a[c] += pfw[((c * 2 + ci) * 3 + ky) * 3 + kx] * v;
        }
      }
    const int base = lane & ~3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int pix = 0; pix < 4; ++pix) in[c * 4 + pix] = __shfl(a[c], base + pix, 64);   // (c, dy, dx) order = conv weight order
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int dy = 0; dy < PATCH; ++dy)
#pragma unroll
        for (int dx = 0; dx < PATCH; ++dx)
          in[(c * PATCH + dy) * PATCH + dx] = img[(((size_t)b * cin + c) * Hi + th * PATCH + dy) * Wi + tw * PATCH + dx];
  }
  // k outermost: a lane's CQ channels are contiguous in wt[k][:], so the weights arrive as 16-byte LDS reads (CQ / 4 per k) instead
  // of one ds_read_b32 per multiply; every output still adds its products in the order k = 0 .. KP - 1 (same bits)
  float o[CQ], s = 0.f;
#pragma unroll
  for (int i = 0; i < CQ; i += 4) {
    const float4 b4 = *reinterpret_cast<const float4*>(pe_b + part * CQ + i);
    o[i] = b4.x; o[i + 1] = b4.y; o[i + 2] = b4.z; o[i + 3] = b4.w;
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
#pragma unroll
    for (int i = 0; i < CQ; i += 4) {
      const float4 w4 = *reinterpret_cast<const float4*>(wt + k * C + part * CQ + i);
      o[i] += w4.x * in[k]; o[i + 1] += w4.y * in[k]; o[i + 2] += w4.z * in[k]; o[i + 3] += w4.w * in[k];
    }
  }
#pragma unroll
  for (int i = 0; i < CQ; ++i) s += o[i];
  s += xshfl<1>(s); s += xshfl<2>(s);
  const float mean = s * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CQ; ++i) { const float d = o[i] - mean; q += d * d; }
  q += xshfl<1>(q); q += xshfl<2>(q);
  const float rstd = 1.0f / sqrtf(q * (1.0f / C) + 1e-5f);
  // A lane's six float4 of a token row sit 96 bytes from its neighbour's: stored from the registers, a wave instruction touches 64 partial
  // lines and the write path moved 1.9 x the token bytes (35 MB for 18.9 MB at B = 48).  The wave's 16 finished rows go through a
  // wave-private LDS tile instead (rows padded by one float4 against bank conflicts) and leave as 16 C contiguous floats, 1 KB per store
  // instruction.  Lanes of a token past the end computed the last token again; the row count below keeps them out of memory.
  const int wave = threadIdx.x >> 6;
  float* sw = stg + wave * 16 * LDT;
  const float ik = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.f;
#pragma unroll
  for (int i = 0; i < CQ; i += 4) {
    const int c = part * CQ + i;
    float v[4] = {(o[i] - mean) * rstd * ln_w[c] + ln_b[c], (o[i + 1] - mean) * rstd * ln_w[c + 1] + ln_b[c + 1],
                  (o[i + 2] - mean) * rstd * ln_w[c + 2] + ln_b[c + 2], (o[i + 3] - mean) * rstd * ln_w[c + 3] + ln_b[c + 3]};
    if (p_drop > 0.f) {
      const unsigned long long z0 = drop_z0(seed, (unsigned long long)token * C + c);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= drop_scale_z(z0 + (unsigned long long)r * DROP_PHI, p_drop, ik);
    }
    *reinterpret_cast<float4*>(sw + (lane >> 2) * LDT + c) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the tile is private to the wave: no block barrier
  const long tok0 = (long)blockIdx.x * 64 + wave * 16;
  const long left = ntok - tok0;
  const int nfl = (left >= 16 ? 16 : (left > 0 ? (int)left : 0)) * C;   // floats of this wave's rows that exist
  float* dst = tok + (size_t)tok0 * C;
#pragma unroll
  for (int it = 0; it < C / 16; ++it) {
    const int idx = (it * 64 + lane) * 4;
    const int row = idx / C, col = idx - row * C;
    if (idx < nfl) *reinterpret_cast<float4*>(dst + idx) = *reinterpret_cast<const float4*>(sw + row * LDT + col);
  }
}

// ---------------------------------------------------------------------------------- window attention
// Work unit ("slab") = 64 consecutive window-major tokens of one (image, group): 4 windows of 4x4 or 16 of 2x2 (head dim 16;
// the other shapes run on the matrix cores below).
// Block = 256 threads = 2 slabs x 2 heads, one wave per (slab, head), lane = query row.
// K/V (and Q, for coalescing) of the slab's windows are staged in LDS: rows of CG floats; every lane
// of a window reads the same K/V row at a time (LDS broadcast).  Softmax is online over 16-key chunks.
// HBM-bound: 4*L*C*4 bytes per image per block against 11 MFLOP.
// DROP (training only): attn_drop (pgrm.py:248) multiplies the normalised probabilities by a regenerated mask
// (common.h drop_scale) before P.V; the softmax denominator is over the undropped row.
template <int WS, int D, bool DROP>   // D = head dim; channels per group CG = 2*D (two heads per group)
__global__ __launch_bounds__(256) void k_window_attn(const float* __restrict__ q, const float* __restrict__ kv,
                                                      const float* __restrict__ bias_table, float* __restrict__ out, int B,
                                                      int H, int W, int C, int g, int shift, float p_drop,
                                                      unsigned long long seed) {
  constexpr int N = WS * WS;
  constexpr int CG = 2 * D;
  constexpr int QROWS = 64;                     // queries per slab
  constexpr int KROWS = 64;                     // keys resident per slab (whole windows)
  constexpr int LDR = CG + 4;                   // padded row (floats)
  constexpr int TBL = (2 * WS - 1) * (2 * WS - 1);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tbl = smem;                            // [TBL][2]
  float* base = smem + ((TBL * 2 + 3) & ~3);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slab_in_blk = wave >> 1, head = wave & 1;
  float* Qs = base + slab_in_blk * (QROWS + 2 * KROWS) * LDR;
  float* Ks = Qs + QROWS * LDR;
  float* Vs = Ks + KROWS * LDR;
  int* reg_s = reinterpret_cast<int*>(base + 2 * (QROWS + 2 * KROWS) * LDR) + slab_in_blk * KROWS;

  const int L = H * W;
  const int slabs_per_img = L / QROWS;
  const long slab = (long)blockIdx.x * 2 + slab_in_blk;
  const int b = slab / slabs_per_img;
  const int t0 = (slab % slabs_per_img) * QROWS;        // first window-major token of the slab
  const int nWc = W / WS;
  const bool active = b < B;

  for (int i = threadIdx.x; i < TBL * 2; i += 256) tbl[i] = bias_table[i];

  const int k0 = t0;      // key range = the slab's own (whole) windows
  // ---- stage Q (64 rows), K, V (KROWS rows) of this slab: the 128 threads of the slab's two waves cooperate
  if (active) {
    const int tl = threadIdx.x & 127;
    constexpr int V4 = CG / 4;
    for (int i = tl; i < KROWS * V4; i += 128) {
      const int r = i / V4, c4 = (i % V4) * 4;
      const int t = k0 + r;
      const int win = t / N, n = t % N;
      const int wr = win / nWc, wc = win % nWc;
      const int hr = wr * WS + n / WS, wcol = wc * WS + n % WS;      // rolled-frame coordinates
      const int sh = (hr + shift) % H, sw = (wcol + shift) % W;     // source token (roll by -shift)
      const size_t src = (size_t)b * L + sh * W + sw;
      *reinterpret_cast<float4*>(Ks + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + g * CG + c4);
      *reinterpret_cast<float4*>(Vs + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + C + g * CG + c4);
      if (t >= t0 && t < t0 + QROWS)
        *reinterpret_cast<float4*>(Qs + (t - t0) * LDR + c4) = *reinterpret_cast<const float4*>(q + src * C + g * CG + c4);
      if (c4 == 0) {
        int rh = hr < H - WS ? 0 : (hr < H - shift ? 1 : 2);
        int rw = wcol < W - WS ? 0 : (wcol < W - shift ? 1 : 2);
        reg_s[r] = 3 * rh + rw;
      }
    }
  }
  __syncthreads();
  if (!active) return;

  // ---- lane = query row
  const int tq = t0 + lane;
  const int nq = tq % N;
  const int krow0 = (lane / N) * N;   // first key row (in Ks) of this lane's window
  const int iq = nq / WS, jq = nq % WS;
  const int my_reg = reg_s[tq - k0];
  float qv[D];
  const float scale = 1.0f / sqrtf((float)D);
  const float* qrow = Qs + lane * LDR + head * D;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(qrow + d);
    qv[d] = v.x * scale; qv[d + 1] = v.y * scale; qv[d + 2] = v.z * scale; qv[d + 3] = v.w * scale;
  }
  float o[D];
#pragma unroll
  for (int d = 0; d < D; ++d) o[d] = 0.f;
  float mx = -INFINITY, den = 0.f;
  const unsigned long long mrow = (((unsigned long long)((size_t)b * (C / CG) + g) * 2 + head) * L + tq) * N;
  const float inv_keep = DROP ? 1.0f / (1.0f - p_drop) : 1.0f;
  constexpr int CH = (N < 16) ? N : 16;
  for (int m0 = 0; m0 < N; m0 += CH) {
    float sc[CH];
    float cmax = -INFINITY;
#pragma unroll
    for (int mm = 0; mm < CH; ++mm) {
      const int m = m0 + mm;
      const float* kr = Ks + (krow0 + m) * LDR + head * D;
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < D; d += 4) {
        const float4 kk = *reinterpret_cast<const float4*>(kr + d);
        a += qv[d] * kk.x + qv[d + 1] * kk.y + qv[d + 2] * kk.z + qv[d + 3] * kk.w;
      }
      const int im = m / WS, jm = m % WS;
      a += tbl[((iq - im + WS - 1) * (2 * WS - 1) + (jq - jm + WS - 1)) * 2 + head];
      if (shift > 0 && reg_s[krow0 + m] != my_reg) a += -100.0f;
      sc[mm] = a;
      cmax = fmaxf(cmax, a);
    }
    const float nmx = fmaxf(mx, cmax);
    const float resc = __expf(mx - nmx);   // exp(-inf) = 0 on the first chunk
    den *= resc;
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] *= resc;
#pragma unroll
    for (int mm = 0; mm < CH; ++mm) {
      float p = __expf(sc[mm] - nmx);
      den += p;
      if (DROP) p *= drop_scale(seed, mrow + m0 + mm, p_drop, inv_keep);
      const float* vr = Vs + (krow0 + m0 + mm) * LDR + head * D;
#pragma unroll
      for (int d = 0; d < D; d += 4) {
        const float4 vv = *reinterpret_cast<const float4*>(vr + d);
        o[d] += p * vv.x; o[d + 1] += p * vv.y; o[d + 2] += p * vv.z; o[d + 3] += p * vv.w;
      }
    }
    mx = nmx;
  }
  const float inv = 1.0f / den;
  float* dst = out + ((size_t)b * L + tq) * C + g * CG + head * D;
#pragma unroll
  for (int d = 0; d < D; d += 4)
    *reinterpret_cast<float4*>(dst + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

// ---------------------------------------------------------------------------------- window attention on the matrix cores
// 8x8 windows, head dim 16 (the group that carries 76 % of the attention FLOPs): same block / slab /
// LDS staging as k_window_attn (block = 2 windows x 2 heads, one wave per (window, head)), but QK^T and PV run as
// v_mfma_f32_16x16x4_f32 instead of 64 x 64 x 16 scalar FMAs per lane:
//   S^T tile (16 keys x 16 queries) = K (A operand: rows = keys) . Q^T (B operand: columns = queries); the reduction index of
//   one MFMA is d = 4*kq + s, so one ds_read_b128 per operand tile feeds the 4 k-steps.  Lane (lr, kq) then holds
//   S^T[key = 16t + 4kq + r][query = 16qt + lr]: a query's 64 logits sit in the 16 accumulator values of 4 lanes, and the
//   softmax reduction over keys is a 16-value scan plus two xor-shuffles (16, 32).
//   O^T (16 d x 16 queries) = V^T (A: rows = d) . P (B).  The B operand of reduction step (t, r) is the key 16t + 4kq + r --
//   exactly the accumulator element the lane already holds, so P never leaves its registers (no LDS transpose); V^T comes
//   from the staged V rows with one ds_read_b32 per step, shared by the 4 query tiles.
// The result lands as O[query][d = 4kq + r]: one float4 store per lane and query tile.
template <bool DROP>
__global__ __launch_bounds__(256) void k_window_attn8_mfma(const float* __restrict__ q, const float* __restrict__ kv,
                                                            const float* __restrict__ bias_table, float* __restrict__ out,
                                                            int B, int H, int W, int C, int g, int shift, float p_drop,
                                                            unsigned long long seed) {
  constexpr int WS = 8, D = 16, N = 64, CG = 2 * D, LDR = CG + 4, TBL = (2 * WS - 1) * (2 * WS - 1);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tbl = smem;                            // [TBL][2]
  float* base = smem + ((TBL * 2 + 3) & ~3);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slab_in_blk = wave >> 1, head = wave & 1;
  float* Qs = base + slab_in_blk * 3 * N * LDR;
  float* Ks = Qs + N * LDR;
  float* Vs = Ks + N * LDR;
  int* reg_s = reinterpret_cast<int*>(base + 2 * 3 * N * LDR) + slab_in_blk * N;

  const int L = H * W;
  const int slabs_per_img = L / N;
  const long slab = (long)blockIdx.x * 2 + slab_in_blk;
  const int b = slab / slabs_per_img;
  const int t0 = (slab % slabs_per_img) * N;         // first window-major token of the window
  const int nWc = W / WS;
  const bool active = b < B;

  for (int i = threadIdx.x; i < TBL * 2; i += 256) tbl[i] = bias_table[i];
  if (active) {
    const int tl = threadIdx.x & 127;
    constexpr int V4 = CG / 4;
    for (int i = tl; i < N * V4; i += 128) {
      const int r = i / V4, c4 = (i % V4) * 4;
      const int t = t0 + r;
      const int win = t / N, n = t % N;
      const int hr = (win / nWc) * WS + n / WS, wcol = (win % nWc) * WS + n % WS;       // rolled-frame coordinates
      const size_t src = (size_t)b * L + ((hr + shift) % H) * W + (wcol + shift) % W;  // source token (roll by -shift)
      *reinterpret_cast<float4*>(Ks + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + g * CG + c4);
      *reinterpret_cast<float4*>(Vs + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + C + g * CG + c4);
      *reinterpret_cast<float4*>(Qs + r * LDR + c4) = *reinterpret_cast<const float4*>(q + src * C + g * CG + c4);
      if (c4 == 0) {
        const int rh = hr < H - WS ? 0 : (hr < H - shift ? 1 : 2), rw = wcol < W - WS ? 0 : (wcol < W - shift ? 1 : 2);
        reg_s[r] = 3 * rh + rw;
      }
    }
  }
  __syncthreads();
  if (!active) return;

  const int lr = lane & 15, kq = lane >> 4;
  const float scale = 0.25f;                       // 16^-0.5
  // ---- S^T = K . Q^T
  f32x4 kf[4], qf[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    kf[t] = *reinterpret_cast<const f32x4*>(Ks + (16 * t + lr) * LDR + head * D + 4 * kq);
    qf[t] = *reinterpret_cast<const f32x4*>(Qs + (16 * t + lr) * LDR + head * D + 4 * kq);
    qf[t] *= scale;
  }
  f32x4 sacc[4][4];       // [key tile][query tile]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) a = mfma16(kf[t][s4], qf[qt][s4], a);
      sacc[t][qt] = a;
    }
  // ---- + relative position bias, shift mask; softmax over the keys of each query column
  float inv[4];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    const int nq = 16 * qt + lr, iq = nq / WS, jq = nq % WS;
    const int my_reg = reg_s[nq];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * t + 4 * kq + r, im = m / WS, jm = m % WS;
        float a = sacc[t][qt][r] + tbl[((iq - im + WS - 1) * (2 * WS - 1) + (jq - jm + WS - 1)) * 2 + head];
        if (shift > 0 && reg_s[m] != my_reg) a += -100.0f;
        sacc[t][qt][r] = a;
        mx = fmaxf(mx, a);
      }
    mx = fmaxf(mx, xshfl<16>(mx));
    mx = fmaxf(mx, xshfl<32>(mx));
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(sacc[t][qt][r] - mx);
        sacc[t][qt][r] = p;
        den += p;
      }
    den += xshfl<16>(den);
    den += xshfl<32>(den);
    inv[qt] = 1.0f / den;
    if (DROP) {      // attn_drop (pgrm.py:248): same mask index as k_window_attn -- query row base + key
      const unsigned long long mrow = (((unsigned long long)((size_t)b * (C / CG) + g) * 2 + head) * L + t0 + nq) * N;
      const float inv_keep = 1.0f / (1.0f - p_drop);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sacc[t][qt][r] *= drop_scale(seed, mrow + 16 * t + 4 * kq + r, p_drop, inv_keep);
    }
  }
  // ---- O^T = V^T . P
  f32x4 oacc[4];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) oacc[qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float vt = Vs[(16 * t + 4 * kq + r) * LDR + head * D + lr];      // V^T[d = lr][key = 16t + 4kq + r]
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) oacc[qt] = mfma16(vt, sacc[t][qt][r], oacc[qt]);
    }
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    const int tq = t0 + 16 * qt + lr;
    float* dst = out + ((size_t)b * L + tq) * C + g * CG + head * D + 4 * kq;
    *reinterpret_cast<float4*>(dst) = make_float4(oacc[qt][0] * inv[qt], oacc[qt][1] * inv[qt], oacc[qt][2] * inv[qt], oacc[qt][3] * inv[qt]);
  }
}

template <bool DROP>
int launch_window_attn8_mfma(const float* q, const float* kv, const float* table, float* out, int B, int H, int W, int C, int g,
                             int shift, float p_drop, unsigned long long seed, hipStream_t st) {
  constexpr int N = 64, LDR = 36, TBL = 15 * 15;
  const size_t smem = (size_t)(((TBL * 2 + 3) & ~3) + 2 * 3 * N * LDR) * 4 + 2 * N * 4;
  dpmn_lds_optin<k_window_attn8_mfma<DROP>>(smem);
  const long slabs = (long)B * (H * W / 64);
  // per (window, head): QK^T + PV = 4 * N^2 * d FLOPs; q, k, v read + out written for this group's 32 channels
  ProfScope prof(PT_WATTN8, st, 4.0 * 64 * 16 * 2 * (double)B * H * W, 4.0 * 4 * 32 * (double)B * H * W);
  hipLaunchKernelGGL((k_window_attn8_mfma<DROP>), dim3((unsigned)((slabs + 1) / 2)), dim3(256), smem, st, q, kv, table, out, B, H, W, C, g, shift,
                     p_drop, seed);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}


// ---------------------------------------------------------------------------------- window attention on MFMA, head dim 32
// The stress configuration (BASELINE.json configs[4]: dim 192 = 3 groups x 2 heads x 32, windows 4 / 8 / 16) spent 44 ms of its
// 311 ms step in the scalar kernel above (VALU-bound: a lane walks every key of its query).  Same scheme as the 8x8 kernel, with
// the window size and the head dim as template parameters:
//   * one "key set" per block: a 64-token slab (4 windows of 4x4, or one 8x8 window; two slabs per block) or one 16x16 window
//     (256 tokens, 139 KB of K / V in LDS, eight waves);
//   * a wave = (64-query slab, head) walks its 4 query tiles; per tile S^T = K Q^T over the KT key tiles the tile's windows
//     cover (1, 4, 16), Q read straight from global memory in operand order, P kept in the accumulator registers, O^T = V^T P.
// Relative-position bias and shift mask are looked up per logit like in the scalar kernel (pgrm.py:234-243).
// DROP: attn_drop (pgrm.py:248) on the normalised probabilities, as in the other window-attention kernels (counter-based masks).
template <int WS, int D, bool DROP = false>
__global__ __launch_bounds__((WS == 16 ? 512 : 256)) void k_window_attn_mfma(const float* __restrict__ q, const float* __restrict__ kv,
                                                                             const float* __restrict__ bias_table, float* __restrict__ out,
                                                                             int B, int H, int W, int C, int g, int shift, float p_drop = 0.f,
                                                                             unsigned long long seed = 0ull) {
  constexpr int N = WS * WS, CG = 2 * D, DC = D / 16, LDR = CG + 4, TBL = (2 * WS - 1) * (2 * WS - 1);
  constexpr int ROWS = WS == 16 ? 256 : 64;            // tokens of one key set
  constexpr int SETS = WS == 16 ? 1 : 2;               // key sets per block
  constexpr int KT = N >= 64 ? N / 16 : 1;             // key tiles a query tile attends to
  constexpr int TH = WS == 16 ? 512 : 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tbl = smem;                                   // [TBL][2]
  float* base = smem + ((TBL * 2 + 3) & ~3);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, kq = lane >> 4;
  const int set_in_blk = WS == 16 ? 0 : wave >> 1, head = wave & 1;
  const int slab_in_set = WS == 16 ? wave >> 1 : 0;    // 64-query slab of this wave inside the key set
  float* Ks = base + set_in_blk * 2 * ROWS * LDR;
  float* Vs = Ks + ROWS * LDR;
  int* reg_s = reinterpret_cast<int*>(base + SETS * 2 * ROWS * LDR) + set_in_blk * ROWS;
  const int L = H * W;
  const int sets_per_img = L / ROWS;
  const long set = (long)blockIdx.x * SETS + set_in_blk;
  const int b = (int)(set / sets_per_img);
  const int t0 = (int)(set % sets_per_img) * ROWS;     // first window-major token of the key set
  const int nWc = W / WS;
  const bool active = b < B;
  for (int i = threadIdx.x; i < TBL * 2; i += TH) tbl[i] = bias_table[i];
  // source row (roll by -shift, window partition; pgrm.py:209-213) of window-major token t of image b
  auto src_row = [&](int t, int& hr, int& wcol) {
    const int win = t / N, n = t % N;
    hr = (win / nWc) * WS + n / WS;
    wcol = (win % nWc) * WS + n % WS;
    return (size_t)b * L + ((hr + shift) % H) * W + (wcol + shift) % W;
  };
  if (active) {
    constexpr int V4 = CG / 4, TPS = TH / SETS;        // threads staging one key set
    const int tl = threadIdx.x % TPS;
    for (int i = tl; i < ROWS * V4; i += TPS) {
      const int r = i / V4, c4 = (i % V4) * 4;
      int hr, wcol;
      const size_t src = src_row(t0 + r, hr, wcol);
      *reinterpret_cast<float4*>(Ks + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + g * CG + c4);
      *reinterpret_cast<float4*>(Vs + r * LDR + c4) = *reinterpret_cast<const float4*>(kv + src * 2 * C + C + g * CG + c4);
      if (c4 == 0) {
        const int rh = hr < H - WS ? 0 : (hr < H - shift ? 1 : 2), rw = wcol < W - WS ? 0 : (wcol < W - shift ? 1 : 2);
        reg_s[r] = 3 * rh + rw;
      }
    }
  }
  __syncthreads();
  if (!active) return;
  const float scale = D == 32 ? 0.17677669529663687f : 0.25f;      // head_dim ** -0.5
#pragma unroll 1
  for (int qt = 0; qt < 4; ++qt) {
    const int rq = 64 * slab_in_set + 16 * qt + lr;    // my query's row inside the key set
    int hr_, wc_;
    const size_t qsrc = src_row(t0 + rq, hr_, wc_);
    f32x4 qf[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      qf[dc] = *reinterpret_cast<const f32x4*>(q + qsrc * C + g * CG + head * D + 16 * dc + 4 * kq);
      qf[dc] *= scale;
    }
    const int kbase = WS == 16 ? 0 : (WS == 8 ? 0 : 16 * qt);      // first key row of the windows this query tile sees
    f32x4 sacc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(Ks + (kbase + 16 * kt + lr) * LDR + head * D + 16 * dc + 4 * kq);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) a = mfma16(kf[s4], qf[dc][s4], a);
      }
      sacc[kt] = a;
      if (KT > 4) __builtin_amdgcn_sched_barrier(0);      // 16 key tiles: keep hipcc from hoisting every operand read to the top (spills)
    }
    // + relative position bias, shift mask; softmax over the keys of query column lr
    const int nq = rq % N, iq = nq / WS, jq = nq % WS;
    const int my_reg = reg_s[rq];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = kbase + 16 * kt + 4 * kq + r, m = krow % N, im = m / WS, jm = m % WS;
        float a = sacc[kt][r] + tbl[((iq - im + WS - 1) * (2 * WS - 1) + (jq - jm + WS - 1)) * 2 + head];
        if (shift > 0 && reg_s[krow] != my_reg) a += -100.0f;
        if (WS == 4 && (krow >> 4) != (rq >> 4)) a = -INFINITY;      // (never: a 4x4 query tile is exactly one window)
        sacc[kt][r] = a;
        mx = fmaxf(mx, a);
        if (KT > 4 && r == 3) __builtin_amdgcn_sched_barrier(0);
      }
    mx = fmaxf(mx, xshfl<16>(mx));
    mx = fmaxf(mx, xshfl<32>(mx));
    float den = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pexp = __expf(sacc[kt][r] - mx);
        sacc[kt][r] = pexp;
        den += pexp;
      }
    den += xshfl<16>(den);
    den += xshfl<32>(den);
    const float inv = 1.0f / den;
    if (DROP) {      // mask element ((((b G + g) 2 + head) L + window-major query token) N + key row in the window), include/dpmn_hip.h
      const float inv_keep = 1.0f / (1.0f - p_drop);
      const unsigned long long mrow = ((((unsigned long long)b * (C / CG) + g) * 2 + head) * L + t0 + rq) * N;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) sacc[kt][r] *= drop_scale(seed, mrow + (kbase + 16 * kt + 4 * kq + r) % N, p_drop, inv_keep);
    }
    // O^T = V^T . P: A = V^T[d = 16 dt + lr][key], B = P (the accumulator registers)
    f32x4 oacc[DC];
#pragma unroll
    for (int dt = 0; dt < DC; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vrow = Vs + (kbase + 16 * kt + 4 * kq + r) * LDR + head * D + lr;
#pragma unroll
        for (int dt = 0; dt < DC; ++dt) oacc[dt] = mfma16(vrow[16 * dt], sacc[kt][r], oacc[dt]);
        if (KT > 4 && r == 3) __builtin_amdgcn_sched_barrier(0);
      }
    float* dst = out + ((size_t)b * L + t0 + rq) * C + g * CG + head * D + 4 * kq;
#pragma unroll
    for (int dt = 0; dt < DC; ++dt)
      *reinterpret_cast<float4*>(dst + 16 * dt) = make_float4(oacc[dt][0] * inv, oacc[dt][1] * inv, oacc[dt][2] * inv, oacc[dt][3] * inv);
  }
}

template <int WS, int D, bool DROP = false>
int launch_window_attn_mfma(const float* q, const float* kv, const float* table, float* out, int B, int H, int W, int C, int g,
                            int shift, hipStream_t st, float p_drop = 0.f, unsigned long long seed = 0ull) {
  constexpr int N = WS * WS, CG = 2 * D, LDR = CG + 4, TBL = (2 * WS - 1) * (2 * WS - 1), ROWS = WS == 16 ? 256 : 64, SETS = WS == 16 ? 1 : 2;
  const size_t smem = (size_t)(((TBL * 2 + 3) & ~3) + SETS * 2 * ROWS * LDR) * 4 + (size_t)SETS * ROWS * 4;
  dpmn_lds_optin<k_window_attn_mfma<WS, D, DROP>>(smem);
  const long sets = (long)B * (H * W / ROWS);
  ProfScope prof(PT_WATTN_MFMA32, st, 4.0 * N * D * 2 * (double)B * H * W, 4.0 * 4 * CG * (double)B * H * W);
  hipLaunchKernelGGL((k_window_attn_mfma<WS, D, DROP>), dim3((unsigned)((sets + SETS - 1) / SETS)), dim3(WS == 16 ? 512 : 256), smem, st, q, kv, table,
                     out, B, H, W, C, g, shift, p_drop, seed);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

template <int WS, int D, bool DROP>
int launch_window_attn(const float* q, const float* kv, const float* table, float* out, int B, int H, int W, int C, int g,
                       int shift, float p_drop, unsigned long long seed, hipStream_t st) {
  constexpr int N = WS * WS, CG = 2 * D, KROWS = 64, LDR = CG + 4, TBL = (2 * WS - 1) * (2 * WS - 1);
  const size_t smem = (size_t)(((TBL * 2 + 3) & ~3) + 2 * (64 + 2 * KROWS) * LDR) * 4 + 2 * KROWS * 4;
  dpmn_lds_optin<k_window_attn<WS, D, DROP>>(smem);
  const long slabs = (long)B * (H * W / 64);
  ProfScope prof(PT_WATTN_SCALAR, st, 4.0 * N * D * 2 * (double)B * H * W, 4.0 * 4 * CG * (double)B * H * W);
  hipLaunchKernelGGL((k_window_attn<WS, D, DROP>), dim3((unsigned)((slabs + 1) / 2)), dim3(256), smem, st, q, kv, table, out, B, H, W,
                     C, g, shift, p_drop, seed);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

// ---------------------------------------------------------------------------------- SK gate
// per image: S = mean_t GELU(feats) (from per-block partials) -> fc1 -> GELU -> fc2 -> softmax over groups
// One block of 512 threads per image, and a pure latency chain: so every global read of the block is requested before anything is
// waited for.  Waves 0-3 sum the partials as FOUR chains per channel (chain q adds partials q, q + 4, ... in that order, chain 0 the
// leftover ones behind its own; S = ((s0 + s1) + (s2 + s3)) / L -- the grouping a single thread per channel used before, same
// bits), each chain's loads issued together; waves 4-7 meanwhile copy both weight matrices and both biases into LDS, twelve loads
// per lane in flight (clamped index, predicated LDS store: no branch around a load), so that the two Linear layers read LDS.
constexpr int SKG_T = 512, SKG_STAGE = 12;
__global__ __launch_bounds__(SKG_T) void k_sk_gate(const float* __restrict__ partial, int parts_per_image, int L, const float* __restrict__ fc1_w,
                          const float* __restrict__ fc1_b, const float* __restrict__ fc2_w, const float* __restrict__ fc2_b,
                          float* __restrict__ attn_vec, int C, int G, int dmid) {
  extern __shared__ float sm[];
  float* S = sm;                 // [C]
  float* Z = sm + C;             // [dmid]
  float* A = Z + dmid;           // [C]
  float* Q = A + C;              // [4][C] the four chains
  float* W1 = Q + 4 * C;         // [dmid][C] | [C][dmid] | fc1_b [dmid] | fc2_b [C], one flat index space
  const int nw = dmid * C;
  float* W2 = W1 + nw;
  float* B1 = W2 + nw;
  float* B2 = B1 + dmid;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < SKG_T / 2) {
    const int p4 = parts_per_image & ~3;
    for (int i = tid; i < 4 * C; i += SKG_T / 2) {
      const int q = i / C, c = i - q * C;
      const float* pp = partial + (size_t)b * parts_per_image * C + c;
      float s = 0.f;
#pragma unroll 8
      for (int p = q; p < p4; p += 4) s += pp[(size_t)p * C];
      if (q == 0)
        for (int p = p4; p < parts_per_image; ++p) s += pp[(size_t)p * C];
      Q[i] = s;
    }
  } else {
    const int n = 2 * nw + dmid + C, t = tid - SKG_T / 2;
    for (int i0 = t; i0 < n; i0 += SKG_STAGE * (SKG_T / 2)) {
      float v[SKG_STAGE];
#pragma unroll
      for (int u = 0; u < SKG_STAGE; ++u) {
        int i = i0 + u * (SKG_T / 2);
        i = i < n ? i : n - 1;
        const float* src = i < nw ? fc1_w + i : (i < 2 * nw ? fc2_w + (i - nw) : (i < 2 * nw + dmid ? fc1_b + (i - 2 * nw) : fc2_b + (i - 2 * nw - dmid)));
        v[u] = *src;
      }
#pragma unroll
      for (int u = 0; u < SKG_STAGE; ++u) {
        const int i = i0 + u * (SKG_T / 2);
        if (i < n) W1[i] = v[u];
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += SKG_T) S[c] = ((Q[c] + Q[C + c]) + (Q[2 * C + c] + Q[3 * C + c])) / (float)L;
  __syncthreads();
  // fc1: 8 lanes per output, each sums an eighth of the C products, then a 3-step shuffle reduction
  for (int j0 = 0; j0 < dmid; j0 += SKG_T / 8) {
    const int j = j0 + tid / 8, part = tid & 7;
    float a = 0.f;
    if (j < dmid)
      for (int c = part; c < C; c += 8) a += W1[j * C + c] * S[c];
    a += xshfl<1>(a); a += xshfl<2>(a); a += xshfl<4>(a);
    if (j < dmid && part == 0) Z[j] = gelu_erf(a + B1[j]);
  }
  __syncthreads();
  for (int c = tid; c < C; c += SKG_T) {
    float a = B2[c];
#pragma unroll 8
    for (int j = 0; j < dmid; ++j) a += W2[c * dmid + j] * Z[j];
    A[c] = a;
  }
  __syncthreads();
  const int cg = C / G;
  for (int c = tid; c < cg; c += SKG_T) {
    float mx = -INFINITY;
    for (int g = 0; g < G; ++g) mx = fmaxf(mx, A[g * cg + c]);
    float den = 0.f;
    for (int g = 0; g < G; ++g) den += expf(A[g * cg + c] - mx);
    for (int g = 0; g < G; ++g) attn_vec[((size_t)b * G + g) * cg + c] = expf(A[g * cg + c] - mx) / den;
  }
}

// ---------------------------------------------------------------------------------- depthwise 3x3 + GELU
// planes of r x r (raw reinterpretation of the (B, L, Ch) fc1 output, quirk Q2); one block per 4 planes
// apply_gelu: 0 = g holds the conv output, 1 = g holds GELU(conv), 2 = g holds the conv output AND g2 holds GELU(conv) (the
// training forward keeps the pre-activation for the backward: one pass instead of conv + a separate activation kernel);
// in_gelu: the input is a pre-activation, GELU is applied on the way into the LDS tile (fc1's GELU, pgrm.py:33)
// 32 x 32 planes (the Mlp of the 16 x 64 -> 32 x 128 stacks) take k_dwconv_gelu_r32 below; this is the kernel of every other size:
// a wave takes a BAND of rb rows of a plane (rb = r: the whole plane) with one halo row above and below,
// re-read (and re-activated) from the neighbouring bands -- 64 x 64 planes (the stress stack) as whole-plane tiles need 19 KB of LDS per
// wave, 8 waves per CU, and ran at 0.34 of the HBM rate; 16-row bands need 5 KB
__global__ __launch_bounds__(256) void k_dwconv_gelu(const float* __restrict__ y, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ g, int Ch, int r,
                                                      long planes, int apply_gelu, float* __restrict__ g2, int in_gelu,
                                                      float p_drop, unsigned long long seed, int rb) {
  // p_drop > 0 (with in_gelu): nn.Dropout between fc1's GELU and the conv (pgrm.py:34) -- the mask is a pure function of
  // (seed, element index), so it is applied on load instead of through a materialised activated tensor
  const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  // per wave: one band in an LDS tile of (rb+2) rows x LD = r+8 floats; the plane starts at column 4 so that rows are
  // 16-byte aligned for float4 traffic (global loads / stores and the centre taps); r % 4 == 0
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (rb <= 0) rb = r;
  const int nb = r / rb;
  const long vplane = (long)blockIdx.x * 4 + wave;
  const long plane = vplane / nb;
  const int y0 = (int)(vplane % nb) * rb;
  const bool valid = plane < planes;
  const int c = valid ? (int)(plane % Ch) : 0;
  const int LD = r + 8, r4 = r >> 2;
  float* t = sm + wave * (rb + 2) * LD;
  if (valid) {
    const float* src = y + plane * r * r;
    // tile row j holds plane row y0 - 1 + j
    const int nld = (rb + 2) * r4;
#pragma unroll 4
    for (int it = 0; it < (nld + 63) / 64; ++it) {
      const int i = lane + 64 * it;
      if (i >= nld) break;
      const int j = i / r4, x4 = (i - j * r4) * 4;
      const int yy = y0 - 1 + j;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (yy >= 0 && yy < r) {
        v = *reinterpret_cast<const float4*>(src + yy * r + x4);
        if (in_gelu) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
        if (p_drop > 0.f) {
          const unsigned long long e0 = (unsigned long long)(plane * r * r + yy * r + x4);
          const unsigned long long z0 = drop_z0(seed, e0);
          v.x *= drop_scale_z(z0, p_drop, inv_keep); v.y *= drop_scale_z(z0 + DROP_PHI, p_drop, inv_keep);
          v.z *= drop_scale_z(z0 + 2 * DROP_PHI, p_drop, inv_keep); v.w *= drop_scale_z(z0 + 3 * DROP_PHI, p_drop, inv_keep);
        }
      }
      *reinterpret_cast<float4*>(t + j * LD + 4 + x4) = v;
    }
    for (int i = lane; i < rb + 2; i += 64) { t[i * LD + 3] = 0.f; t[i * LD + 4 + r] = 0.f; }   // left / right halo columns
  }
  // the tile is private to the wave (LDS operations of one wave execute in order): no block barrier
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (!valid) return;
  float k[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) k[i] = w[c * 9 + i];
  const float bv = bias[c];
  float* dst = g + plane * r * r + (size_t)y0 * r;
  for (int i = lane; i < rb * r4; i += 64) {
    const int yy = i / r4, x4 = (i - yy * r4) * 4;
    float a[4] = {bv, bv, bv, bv};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float* p = t + (yy + ky) * LD + 4 + x4;
      const float4 m = *reinterpret_cast<const float4*>(p);
      const float l = p[-1], rr = p[4];
      const float k0 = k[ky * 3], k1 = k[ky * 3 + 1], k2 = k[ky * 3 + 2];
      a[0] += k0 * l + k1 * m.x + k2 * m.y;
      a[1] += k0 * m.x + k1 * m.y + k2 * m.z;
      a[2] += k0 * m.y + k1 * m.z + k2 * m.w;
      a[3] += k0 * m.z + k1 * m.w + k2 * rr;
    }
    if (apply_gelu == 2) {
      *reinterpret_cast<float4*>(dst + yy * r + x4) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(g2 + plane * r * r + (size_t)(y0 + yy) * r + x4) = make_float4(gelu_erf(a[0]), gelu_erf(a[1]), gelu_erf(a[2]), gelu_erf(a[3]));
      continue;
    }
    if (apply_gelu) {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = gelu_erf(a[q]);
    }
    *reinterpret_cast<float4*>(dst + yy * r + x4) = make_float4(a[0], a[1], a[2], a[3]);
  }
}

// 32 x 32 planes, streaming form: a wave walks planes wave, wave + nw, wave + 2 nw, ... (nw = waves of the grid; the launcher sizes the grid
// so that every wave gets the same count) with the NEXT plane's four float4 in registers while it commits, convolves and stores
// this one.  The prefetch is issued before the stores of the current plane and consumed after them: vmcnt retires in order, so the
// wait in front of the next commit leaves the stores outstanding.  Straight-line body (MODE is a template parameter, the prefetch
// of the last plane is peeled off, not predicated), weights by scalar loads (the plane index is wave-uniform): no join after a
// branch with a memory operation, hence no vmcnt(0) drain ("What hipcc's waitcnt insertion needs").
// Per element the operations and their order are those of k_dwconv_gelu: same bits.  MODE = apply_gelu of that kernel.
template <int MODE, bool MORE>
__device__ __forceinline__ void dwconv32_plane(float* __restrict__ t, float4 (&pre)[4], const float* __restrict__ y, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ g, float* __restrict__ g2, int Ch,
                                               int plane, int next, int lane, int in_gelu, float p_drop, float inv_keep,
                                               unsigned long long seed) {
  constexpr int LD = 40;
  const int c = plane % Ch;
  float k[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) k[i] = w[c * 9 + i];
  const float bv = bias[c];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = lane + 64 * it;
    const int j = i >> 3, x4 = (i & 7) * 4;
    float4 v = pre[it];
    if (in_gelu) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
    if (p_drop > 0.f) {
      const unsigned long long z0 = drop_z0(seed, (unsigned long long)plane * 1024 + 4 * i);
      v.x *= drop_scale_z(z0, p_drop, inv_keep); v.y *= drop_scale_z(z0 + DROP_PHI, p_drop, inv_keep);
      v.z *= drop_scale_z(z0 + 2 * DROP_PHI, p_drop, inv_keep); v.w *= drop_scale_z(z0 + 3 * DROP_PHI, p_drop, inv_keep);
    }
    *reinterpret_cast<float4*>(t + (j + 1) * LD + 4 + x4) = v;
  }
  if (MORE) {
    const float* src = y + (size_t)next * 1024;
#pragma unroll
    for (int it = 0; it < 4; ++it) pre[it] = *reinterpret_cast<const float4*>(src + 4 * (lane + 64 * it));
  }
  // the tile is private to the wave (LDS operations of one wave execute in order): no block barrier
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  float* dst = g + (size_t)plane * 1024;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = lane + 64 * it;
    const int yy = i >> 3, x4 = (i & 7) * 4;
    float a[4] = {bv, bv, bv, bv};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float* p = t + (yy + ky) * LD + 4 + x4;
      const float4 m = *reinterpret_cast<const float4*>(p);
      const float l = p[-1], rr = p[4];
      const float k0 = k[ky * 3], k1 = k[ky * 3 + 1], k2 = k[ky * 3 + 2];
      a[0] += k0 * l + k1 * m.x + k2 * m.y;
      a[1] += k0 * m.x + k1 * m.y + k2 * m.z;
      a[2] += k0 * m.y + k1 * m.z + k2 * m.w;
      a[3] += k0 * m.z + k1 * m.w + k2 * rr;
    }
    if (MODE == 2) {
      *reinterpret_cast<float4*>(dst + 4 * i) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(g2 + (size_t)plane * 1024 + 4 * i) = make_float4(gelu_erf(a[0]), gelu_erf(a[1]), gelu_erf(a[2]), gelu_erf(a[3]));
    } else {
      if (MODE == 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = gelu_erf(a[q]);
      }
      *reinterpret_cast<float4*>(dst + 4 * i) = make_float4(a[0], a[1], a[2], a[3]);
    }
  }
  // the next commit overwrites the tile these reads came from (same wave, in order)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <int MODE>
__global__ __launch_bounds__(256) void k_dwconv_gelu_r32(const float* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ g, float* __restrict__ g2,
                                                          int Ch, int planes, int in_gelu, float p_drop, unsigned long long seed) {
  constexpr int LD = 40;
  __shared__ __attribute__((aligned(16))) float sm[4 * 34 * LD];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const int nw = (int)gridDim.x * 4;
  int plane = (int)blockIdx.x * 4 + wave;
  if (plane >= planes) return;                   // wave-uniform; the kernel has no block barrier
  float* t = sm + wave * 34 * LD;
  // zero halo, written once: rows 0 and 33, columns 3 and 36 (the commits only touch rows 1 .. 32, columns 4 .. 35)
  for (int i = lane; i < LD; i += 64) { t[i] = 0.f; t[33 * LD + i] = 0.f; }
  if (lane < 34) { t[lane * LD + 3] = 0.f; t[lane * LD + 36] = 0.f; }
  float4 pre[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) pre[it] = *reinterpret_cast<const float4*>(y + (size_t)plane * 1024 + 4 * (lane + 64 * it));
  for (int next = plane + nw; next < planes; plane = next, next += nw)
    dwconv32_plane<MODE, true>(t, pre, y, w, bias, g, g2, Ch, plane, next, lane, in_gelu, p_drop, inv_keep, seed);
  dwconv32_plane<MODE, false>(t, pre, y, w, bias, g, g2, Ch, plane, plane, lane, in_gelu, p_drop, inv_keep, seed);
}

// ---------------------------------------------------------------------------------- tail
// conv3x3 Cm->Cm + LeakyReLU(0.01) + PixelShuffle(p) + * weight_list_0 + sum_i residual_i * weight_list_i
// output NCHW (B, hid, H*p, W*p); thread = (pixel, output channel)
struct TailResid {
  const float* res[8];
  const float* wl[8];
  int n;
};
__global__ __launch_bounds__(256) void k_tail_conv2(const float* __restrict__ mid, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ wl0, TailResid tr,
                                                     float* __restrict__ out, int B, int H, int W) {
  // hidden 3, patch 2: Cm = 12 channels in and out; thread = one low-res pixel, all 12 outputs
  constexpr int Cm = 12;
  __shared__ __attribute__((aligned(16))) float ws[9 * Cm * Cm];   // [tap][ci][co]
  for (int i = threadIdx.x; i < 9 * Cm * Cm; i += 256) {
    const int co = i % Cm, ci = (i / Cm) % Cm, tap = i / (Cm * Cm);
    ws[i] = w[(co * Cm + ci) * 9 + tap];
  }
  __syncthreads();
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (long)B * H * W) return;
  const int x = pix % W, y = (pix / W) % H, b = pix / ((long)W * H);
  float a[Cm];
#pragma unroll
  for (int co = 0; co < Cm; ++co) a[co] = bias[co];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = y + ky - 1;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = x + kx - 1;
      if (xx < 0 || xx >= W) continue;
      const float* src = mid + (((size_t)b * H + yy) * W + xx) * Cm;
      float v[Cm];
#pragma unroll
      for (int q = 0; q < Cm; q += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(src + q);
        v[q] = t4.x; v[q + 1] = t4.y; v[q + 2] = t4.z; v[q + 3] = t4.w;
      }
      const float* wp = ws + (ky * 3 + kx) * Cm * Cm;
#pragma unroll
      for (int ci = 0; ci < Cm; ++ci)
#pragma unroll
        for (int co = 0; co < Cm; co += 4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wp + ci * Cm + co);
          a[co] += v[ci] * w4.x; a[co + 1] += v[ci] * w4.y; a[co + 2] += v[ci] * w4.z; a[co + 3] += v[ci] * w4.w;
        }
    }
  }
  // LeakyReLU(0.01) + PixelShuffle(2): out[b, c, 2y+dy, 2x+dx] = in[b, 4c + 2dy + dx, y, x]; then weight_list / residuals
  const int Ho = 2 * H, Wo = 2 * W;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      float v0 = a[4 * c + 2 * dy], v1 = a[4 * c + 2 * dy + 1];
      v0 = v0 > 0.f ? v0 : 0.01f * v0;
      v1 = v1 > 0.f ? v1 : 0.01f * v1;
      const size_t po = ((size_t)c * Ho + (2 * y + dy)) * Wo + 2 * x;
      const size_t o = (size_t)b * 3 * Ho * Wo + po;
      const float2 l0 = *reinterpret_cast<const float2*>(wl0 + po);
      float2 r = make_float2(v0 * l0.x, v1 * l0.y);
      for (int i = 0; i < tr.n; ++i) {
        const float2 rs = *reinterpret_cast<const float2*>(tr.res[i] + o);
        const float2 li = *reinterpret_cast<const float2*>(tr.wl[i] + po);
        r.x += rs.x * li.x; r.y += rs.y * li.y;
      }
      *reinterpret_cast<float2*>(out + o) = r;
    }
}

// (Cout, Cin, KH, KW) reference conv weight -> (Cout, Kp) implicit-GEMM pack, K index = (ky*KW+kx)*Cin + ci
__global__ void k_pack_conv_w(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int taps, int Kp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Cout * Kp) return;
  const int co = idx / Kp, k = idx % Kp;
  const int tap = k / Cin, ci = k % Cin;
  wp[idx] = tap < taps ? w[((size_t)co * Cin + ci) * taps + tap] : 0.f;
}

}  // namespace

// ================================================================================== C ABI
extern "C" {

int dpmn_patch_embed_ln_f32(const float* img, int cin, const float* pf_w, const float* pf_b, const float* pe_w,
                            const float* pe_b, const float* ln_w, const float* ln_b, float* tokens, int B, int Hi, int Wi,
                            int patch, int C, dpmn_stream_t stream) {
  return dpmn_patch_embed_ln_drop_f32(img, cin, pf_w, pf_b, pe_w, pe_b, ln_w, ln_b, tokens, B, Hi, Wi, patch, C, 0.f, 0ull, stream);
}

int dpmn_patch_embed_ln_drop_f32(const float* img, int cin, const float* pf_w, const float* pf_b, const float* pe_w,
                                 const float* pe_b, const float* ln_w, const float* ln_b, float* tokens, int B, int Hi, int Wi,
                                 int patch, int C, float p_drop, unsigned long long seed, dpmn_stream_t stream) {
  DPMN_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "patch_embed: drop probability must be in [0, 1)");
  DPMN_REQUIRE(img && pe_w && pe_b && ln_w && ln_b && tokens, "patch_embed: null pointer");
  DPMN_REQUIRE(patch >= 1 && patch <= 4 && Hi % patch == 0 && Wi % patch == 0, "patch_embed: bad patch size");
  DPMN_REQUIRE((pf_w != nullptr) || cin >= 3, "patch_embed: need 3 input channels without prior_fusion");
  const long tokens_n = (long)B * (Hi / patch) * (Wi / patch);
  dim3 grid((unsigned)((tokens_n + 63) / 64));
  DPMN_REQUIRE(patch == 2, "patch_embed: built for patch_size=2 (the --patch_size the DPMN recipe uses, README.md:34)");
  DPMN_REQUIRE(pf_w == nullptr || cin == 2, "patch_embed: prior_fusion expects a 2-channel text prior");
  hipStream_t st = as_stream(stream);
#define PE_LAUNCH(CV, FV) hipLaunchKernelGGL((k_patch_embed_ln<CV, 2, FV>), grid, dim3(256), 0, st, img, cin, pf_w, pf_b, pe_w, pe_b, ln_w, ln_b, tokens, B, Hi, Wi, p_drop, seed)
  if (C == 96 && pf_w) PE_LAUNCH(96, true);
  else if (C == 96) PE_LAUNCH(96, false);
  else if (C == 192 && pf_w) PE_LAUNCH(192, true);
  else if (C == 192) PE_LAUNCH(192, false);
  else return dpmn_set_error(DPMN_ERR_ARG, "patch_embed: embed dim must be 96 or 192");
#undef PE_LAUNCH
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_window_attn_f32(const float* q, const float* kv, const float* const* bias_tables, const int* windows,
                         const int* shifts, int n_groups, int heads_per_group, float* out, int B, int H, int W, int C,
                         dpmn_stream_t stream) {
  return dpmn_window_attn_drop_f32(q, kv, bias_tables, windows, shifts, n_groups, heads_per_group, out, B, H, W, C, 0.f, 0ull, stream);
}

int dpmn_window_attn_drop_f32(const float* q, const float* kv, const float* const* bias_tables, const int* windows,
                              const int* shifts, int n_groups, int heads_per_group, float* out, int B, int H, int W, int C,
                              float p_drop, unsigned long long seed, dpmn_stream_t stream) {
  DPMN_REQUIRE(q && kv && bias_tables && windows && shifts && out, "window_attn: null pointer");
  DPMN_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "window_attn: attn_drop must be in [0, 1)");
  DPMN_REQUIRE(heads_per_group == 2, "window_attn: two heads per group (num_heads = 2 * n_groups)");
  DPMN_REQUIRE(C % n_groups == 0, "window_attn: C must divide into groups");
  const int D = C / n_groups / heads_per_group;
  DPMN_REQUIRE((H * W) % 64 == 0, "window_attn: token count must be a multiple of 64");
  hipStream_t st = as_stream(stream);
  for (int g = 0; g < n_groups; ++g) {      // every group is checked before the first launch: a rejected call writes nothing
    const int ws = windows[g], sh = shifts[g];
    DPMN_REQUIRE((D == 16 && (ws == 2 || ws == 4 || ws == 8)) || (D == 32 && (ws == 4 || ws == 8 || ws == 16)),
                 "window_attn: unsupported (window, head_dim); built: {2,4,8}x16, {4,8,16}x32");
    DPMN_REQUIRE(H % ws == 0 && W % ws == 0, "window_attn: padding path (H or W not divisible by window) would crash the reference (quirk Q1)");
    DPMN_REQUIRE(sh >= 0 && sh < ws, "window_attn: shift must be in [0, window)");
  }
  for (int g = 0; g < n_groups; ++g) {
    const int ws = windows[g], sh = shifts[g];
    int rc = DPMN_ERR_ARG;
    if (ws == 8 && D == 16) {
      rc = p_drop > 0.f ? launch_window_attn8_mfma<true>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, p_drop, seed, st)
                        : launch_window_attn8_mfma<false>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, 0.f, 0ull, st);
      if (rc != DPMN_OK) return rc;
      continue;
    }
    if (D == 32 && (ws == 4 || ws == 8 || ws == 16)) {
      if (p_drop > 0.f)
        rc = ws == 4 ? launch_window_attn_mfma<4, 32, true>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st, p_drop, seed)
                     : (ws == 8 ? launch_window_attn_mfma<8, 32, true>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st, p_drop, seed)
                                : launch_window_attn_mfma<16, 32, true>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st, p_drop, seed));
      else
      rc = ws == 4 ? launch_window_attn_mfma<4, 32>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st)
                   : (ws == 8 ? launch_window_attn_mfma<8, 32>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st)
                              : launch_window_attn_mfma<16, 32>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, st));
      if (rc != DPMN_OK) return rc;
      continue;
    }
#define WA_CASE(WSV, DV) if (ws == WSV && D == DV) rc = p_drop > 0.f \
      ? launch_window_attn<WSV, DV, true>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, p_drop, seed, st) \
      : launch_window_attn<WSV, DV, false>(q, kv, bias_tables[g], out, B, H, W, C, g, sh, 0.f, 0ull, st); else
    WA_CASE(2, 16) WA_CASE(4, 16)
    return dpmn_set_error(DPMN_ERR_ARG, "window_attn: unsupported (window, head_dim); built: {2,4,8}x16, {4,8,16}x32");
#undef WA_CASE
    if (rc != DPMN_OK) return rc;
  }
  return DPMN_OK;
}

int dpmn_sk_gate_f32(const float* colsum_partials, int parts_per_image, int L, const float* fc1_w, const float* fc1_b,
                     const float* fc2_w, const float* fc2_b, float* attn_vec, int B, int C, int groups, int dmid,
                     dpmn_stream_t stream) {
  DPMN_REQUIRE(colsum_partials && fc1_w && fc1_b && fc2_w && fc2_b && attn_vec, "sk_gate: null pointer");
  // quirk Q3: at B = 1 the reference's feats_S.squeeze() also drops the batch axis, but the later .view(bs, M, channel, 1, 1)
  // restores it -- same arithmetic as B >= 2 (pinned by the B = 1 stress golden), so no restriction here
  DPMN_REQUIRE(B >= 1 && parts_per_image >= 1 && L >= 1 && C >= 1 && dmid >= 1 && groups >= 1 && C % groups == 0, "sk_gate: bad shape");
  // S, Z, A, four chains, both weight matrices and biases: the kernel reads fc1 / fc2 from LDS only, so 2 C dmid floats must fit (C = 96 /
  // 192 with dmid = C / 6: 15 / 55 KB).  A gate too large for that (C = 768 at dmid = C / 6 would be) is an error, not a slower path: no model of
  // the project has one, and the kernel before this one, which read the weights from global memory, accepted it.
  const size_t smem = ((size_t)7 * C + 2 * dmid + (size_t)2 * dmid * C) * 4;
  DPMN_REQUIRE(smem <= 160 * 1024, "sk_gate: fc1 / fc2 do not fit in LDS");
  dpmn_lds_optin<k_sk_gate>(smem);
  hipLaunchKernelGGL(k_sk_gate, dim3(B), dim3(SKG_T), smem, as_stream(stream), colsum_partials,
                     parts_per_image, L, fc1_w, fc1_b, fc2_w, fc2_b, attn_vec, C, groups, dmid);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

// One launch path for the four entry points.  apply_gelu / in_gelu as in k_dwconv_gelu.  32 x 32 planes take the streaming kernel on a
// grid of at most 7 blocks per CU (21.8 KB of LDS each) in which every wave walks the same number of planes (the last ones one
// less when the count does not divide); every other plane size takes k_dwconv_gelu on whole planes or 16-row bands.
static unsigned dwconv32_grid(long planes) {
  const long cap = 7L * dpmn_cu_count() * 4;       // resident waves (3, 4 and 6 blocks per CU measured slower or equal)
  const long per = (planes + cap - 1) / cap;       // planes per wave
  const long waves = (planes + per - 1) / per;
  return (unsigned)((waves + 3) / 4);
}

static int launch_dwconv(const float* y, const float* w, const float* bias, float* g, float* g2, int apply_gelu, int in_gelu, float p_drop,
                         unsigned long long seed, int B, int Ch, int r, hipStream_t st) {
  const long planes = (long)B * Ch;
  DPMN_REQUIRE(planes >= 1 && planes <= (1L << 30), "dwconv: B * Ch out of range");
  if (r == 32) {
    const dim3 grid(dwconv32_grid(planes));
#define DW32(MODE) hipLaunchKernelGGL(k_dwconv_gelu_r32<MODE>, grid, dim3(256), 0, st, y, w, bias, g, g2, Ch, (int)planes, in_gelu, p_drop, seed)
    if (apply_gelu == 2) DW32(2);
    else if (apply_gelu == 1) DW32(1);
    else DW32(0);
#undef DW32
  } else {
    const int rb = dwconv_band_rows(r);
    const long vplanes = planes * (r / rb);
    const size_t smem = (size_t)4 * (rb + 2) * (r + 8) * 4;
    dpmn_lds_optin<k_dwconv_gelu>(smem);
    hipLaunchKernelGGL(k_dwconv_gelu, dim3((unsigned)((vplanes + 3) / 4)), dim3(256), smem, st, y, w, bias, g, Ch, r, planes, apply_gelu, g2,
                       in_gelu, p_drop, seed, rb);
  }
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_dwconv3x3_gelu_f32(const float* y, const float* w, const float* bias, float* g, int B, int Ch, int r,
                            dpmn_stream_t stream) {
  DPMN_REQUIRE(y && w && bias && g && r >= 4 && r <= 64 && r % 4 == 0, "dwconv: plane side must be a multiple of 4 in [4, 64]");
  ProfScope prof(PT_DWCONV_GELU, as_stream(stream), 18.0 * B * Ch * r * r, 8.0 * B * Ch * r * r);
  return launch_dwconv(y, w, bias, g, nullptr, 1, 0, 0.f, 0ull, B, Ch, r, as_stream(stream));
}

// y holds fc1's PRE-activation: its GELU (pgrm.py:33) is applied on the way into the LDS tile -- once per element, in a kernel that
// waits on HBM anyway -- instead of in the epilogue of the MFMA-bound fc1 GEMM
int dpmn_dwconv3x3_gelu_in_f32(const float* y, const float* w, const float* bias, float* g, int B, int Ch, int r, dpmn_stream_t stream) {
  DPMN_REQUIRE(y && w && bias && g && r >= 4 && r <= 64 && r % 4 == 0, "dwconv: plane side must be a multiple of 4 in [4, 64]");
  ProfScope prof(PT_DWCONV_GELU, as_stream(stream), 18.0 * B * Ch * r * r, 8.0 * B * Ch * r * r);
  return launch_dwconv(y, w, bias, g, nullptr, 1, 1, 0.f, 0ull, B, Ch, r, as_stream(stream));
}

int dpmn_dwconv3x3_f32(const float* y, const float* w, const float* bias, float* g, int B, int Ch, int r, dpmn_stream_t stream) {
  DPMN_REQUIRE(y && w && bias && g && r >= 4 && r <= 64 && r % 4 == 0, "dwconv: plane side must be a multiple of 4 in [4, 64]");
  return launch_dwconv(y, w, bias, g, nullptr, 0, 0, 0.f, 0ull, B, Ch, r, as_stream(stream));
}

int dpmn_dwconv3x3_train_f32(const float* y, const float* w, const float* bias, float* gpre, float* g, int in_gelu, float p_drop,
                             unsigned long long seed, int B, int Ch, int r, dpmn_stream_t stream) {
  DPMN_REQUIRE(y && w && bias && gpre && g && r >= 4 && r <= 64 && r % 4 == 0, "dwconv_train: plane side must be a multiple of 4 in [4, 64]");
  return launch_dwconv(y, w, bias, gpre, g, 2, in_gelu, p_drop, seed, B, Ch, r, as_stream(stream));
}

int dpmn_pgrm_tail_f32(const float* tokens, const float* w0, const float* b0, const float* w1, const float* b1,
                       const float* const* weight_list, const float* const* residuals, int n_residuals, float* mid_ws,
                       float* out, int B, int H, int W, int C, int hidden, int patch, dpmn_stream_t stream) {
  return dpmn_pgrm_tail_reuse_f32(tokens, w0, b0, w1, b1, weight_list, residuals, n_residuals, mid_ws, out, B, H, W, C, hidden, patch, 0, stream);
}

int dpmn_pgrm_tail_reuse_f32(const float* tokens, const float* w0, const float* b0, const float* w1, const float* b1,
                             const float* const* weight_list, const float* const* residuals, int n_residuals, float* mid_ws,
                             float* out, int B, int H, int W, int C, int hidden, int patch, int reuse_pack, dpmn_stream_t stream) {
  DPMN_REQUIRE(tokens && w0 && b0 && w1 && b1 && weight_list && mid_ws && out, "tail: null pointer");
  DPMN_REQUIRE(n_residuals >= 0 && n_residuals <= 8, "tail: at most 8 residuals");
  DPMN_REQUIRE(hidden == 3 && patch == 2 && C % 4 == 0, "tail: built for hidden_size=3, patch_size=2 (super_resolution.py:38-53)");
  const int Cm = hidden * patch * patch;
  const int Kp = ((9 * C + 31) / 32) * 32;
  // mid_ws layout: [B*H*W*Cm mid activations][Cm*Kp packed conv0 weights]
  float* wp = mid_ws + (size_t)B * H * W * Cm;
  if (!reuse_pack) {     // (frozen weights, same workspace: the pack of the previous call is still there, dpmn_pgrm_weights.reuse_folded)
    hipLaunchKernelGGL(k_pack_conv_w, dim3((Cm * Kp + 255) / 256), dim3(256), 0, as_stream(stream), w0, wp, Cm, C, 9, Kp);
    DPMN_CHECK_LAUNCH();
  }
  dpmn_conv_desc d{};
  d.in[0] = tokens; d.cseg[0] = C; d.B = B; d.Hin = H; d.Win = W;
  d.KH = 3; d.KW = 3; d.stride = 1; d.dil_y = 1; d.dil_x = 1; d.pad_y = 1; d.pad_x = 1;
  d.Hp = H; d.Wp = W; d.Hout = H; d.Wout = W; d.ostep = 1;
  d.w = wp; d.bias = b0; d.Cout = Cm; d.out = mid_ws;
  int rc = dpmn_conv2d_nhwc_f32(&d, stream);   // conv_before_upsample[0] on the MFMA implicit-GEMM path
  if (rc != DPMN_OK) return rc;
  TailResid tr{};
  // quirk Q11: residual_list[0] is never added -- the loop starts at 1 (pgrm.py:563)
  tr.n = 0;
  for (int i = 1; i < n_residuals; ++i) {
    tr.res[tr.n] = residuals[i];
    tr.wl[tr.n] = weight_list[i];
    ++tr.n;
  }
  const long pixels = (long)B * H * W;
  hipLaunchKernelGGL(k_tail_conv2, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, as_stream(stream), mid_ws, w1, b1,
                     weight_list[0], tr, out, B, H, W);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
