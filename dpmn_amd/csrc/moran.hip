// Kernels of the native MORAN recogniser (model/moran.py NativeMORAN; reference model/moran/) that are not a conv / GEMM / pool /
// BiLSTM (the prep kernel is k_gray_prep with its plane output, crnn.hip):
//   k_moran_rectify   one pass of MORN (morn.py:63-71 / 74-82) behind the offset head: pool(relu(o)) - pool(relu(-o)) with
//                     MaxPool2d(2, 1) of the Hm x Wm offset map, grid_sample (bilinear, zero padding, align_corners=False) of it on the
//                     identity grid, accumulation into the running offsets, and the zero-padded bilinear warp of the image along y
//   k_moran_split     y1 | y2 = the two channel halves of x[:, ::sy, ::sx, :]: conv1 and downsample of a residual stage's first block
//                     run as ONE conv with concatenated output channels; the (2, 1) stages run it at stride 1 (dpmn_conv_desc has one
//                     scalar stride) and gather the rows here
//   k_moran_decode    the greedy L2R attention decoder (asrn_res.py:127-144 with AttentionCell's test branch), ALL steps in one launch:
//                     a block owns 16 images and keeps the hidden state in LDS; h2h, the GRU's two products and the generator run on
//                     v_mfma_f32_16x16x4_f32 (fp32 in every compute mode), one wave per image does scores / softmax / context
#include "common.h"

namespace {

constexpr int MH = 256;            // hidden size = encoder feature width = embedding width
constexpr int MG = 3 * MH;         // GRU gate rows (r, z, n)
constexpr int M_HP = MH + 4;       // LDS row pitch: the 16 rows of a 16-lane group start 4 banks apart
constexpr int M_MAXT = 64;         // encoder positions (25 for 32 x 100 images): one lane per position
constexpr int M_MAXCLS = 48;       // classes, whole 16-wide tiles (37)

__global__ void k_moran_rectify(const float* __restrict__ omap, const float* __restrict__ plane, const float* __restrict__ gx,
                                const float* __restrict__ gy, const float* __restrict__ acc_in, float* __restrict__ acc_out,
                                float* __restrict__ rect, float* __restrict__ rect4, int B, int H, int W, int Hm, int Wm) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * H * W) return;
  const int x = idx % W, y = (idx / W) % H, b = idx / ((long)W * H);
  const int Hq = Hm - 1, Wq = Wm - 1;            // the pooled map
  const float cx = gx[x], cy = gy[y];
  const float* o = omap + (size_t)b * Hm * Wm;
  // grid_sampler_unnormalize with align_corners=False: ((coord + 1) * size - 1) / 2
  float off = 0.f;
  {
    const float fx = ((cx + 1.f) * (float)Wq - 1.f) / 2.f, fy = ((cy + 1.f) * (float)Hq - 1.f) / 2.f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wx1 = fx - x0f, wx0 = (x0f + 1.f) - fx, wy1 = fy - y0f, wy0 = (y0f + 1.f) - fy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                 // nw, ne, sw, se
      const int px = x0 + (c & 1), py = y0 + (c >> 1);
      if (px < 0 || px >= Wq || py < 0 || py >= Hq) continue;
      float pos = 0.f, neg = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float v = o[(py + (d >> 1)) * Wm + px + (d & 1)];
        pos = fmaxf(pos, v);                      // max of relu(v)
        neg = fmaxf(neg, -v);                     // max of relu(-v)
      }
      off += (pos - neg) * (((c & 1) ? wx1 : wx0) * ((c >> 1) ? wy1 : wy0));
    }
  }
  const float a = acc_in ? acc_in[idx] + off : off;
  acc_out[idx] = a;
  const float fx = ((cx + 1.f) * (float)W - 1.f) / 2.f, fy = ((cy + a + 1.f) * (float)H - 1.f) / 2.f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float wx1 = fx - x0f, wx0 = (x0f + 1.f) - fx, wy1 = fy - y0f, wy0 = (y0f + 1.f) - fy;
  const float* p = plane + (size_t)b * H * W;
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int px = x0 + (c & 1), py = y0 + (c >> 1);
    if (px < 0 || px >= W || py < 0 || py >= H) continue;      // zero padding (also what a non-finite offset falls back to)
    v += p[(size_t)py * W + px] * (((c & 1) ? wx1 : wx0) * ((c >> 1) ? wy1 : wy0));
  }
  rect[idx] = v;
  *reinterpret_cast<float4*>(rect4 + idx * 4) = make_float4(v, 0.f, 0.f, 0.f);
}

__global__ void k_moran_split(const float* __restrict__ x, float* __restrict__ y1, float* __restrict__ y2, int B, int H, int W, int C,
                              int sy, int sx, int Ho, int Wo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 2;            // float4 per pixel of x (2 C channels)
  if (idx >= (long)B * Ho * Wo * C4) return;
  const int c = (idx % C4) * 4;
  const long p = idx / C4;
  const int ox = p % Wo, oy = (p / Wo) % Ho, b = p / ((long)Wo * Ho);
  const float4 v = *reinterpret_cast<const float4*>(x + (((size_t)b * H + (size_t)oy * sy) * W + (size_t)ox * sx) * (2 * C) + c);
  float* dst = c < C ? y1 + (size_t)p * C + c : y2 + (size_t)p * C + (c - C);
  *reinterpret_cast<float4*>(dst) = v;
}

// 16 x 16 tile of A W^T over K = 256: a = this lane's row of A in LDS, w = this lane's row of W in global memory, both already
// advanced by 4 (lane >> 4) floats; the four MFMAs of a 16-wide k chunk walk the float4 element by element (the k order inside a
// chunk is the same permutation on both sides)
__device__ __forceinline__ f32x4 tile_k256(const float* a, const float* __restrict__ w) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int k = 0; k < MH; k += 16) {
    const float4 av = *reinterpret_cast<const float4*>(a + k);
    const float4 wv = *reinterpret_cast<const float4*>(w + k);
    acc0 = mfma16(av.x, wv.x, acc0);
    acc1 = mfma16(av.y, wv.y, acc1);
    acc0 = mfma16(av.z, wv.z, acc0);
    acc1 = mfma16(av.w, wv.w, acc1);
  }
  return acc0 + acc1;
}

// Block = 16 images, 16 waves.  Per step:
//   1  wave q: columns 16 q .. +15 of h2h(h) + b                                        -> ps
//   2  wave q: image q -- e_t = score . tanh(fproj[t] + ps), softmax over t (lane t), context = sum_t alpha_t feats[t]   -> cs
//   3  wave q: hidden units 16 q .. +15 -- the (r, z, n) tiles of context W_ih[:, :256]^T and of h W_hh^T, torch's GRUCell formula
//      with the embedding half of the input product from the table E = char_embeddings W_ih[:, 256:]^T + b_ih         -> hs
//   4  waves 0 .. 2: generator tiles -> logits (global) and lg;  5  one thread per image: arg-max (first maximum), next embedding
__global__ __launch_bounds__(1024) void k_moran_decode(const float* __restrict__ feats, const float* __restrict__ fproj,
                                                        const dpmn_moran_dec_weights w, float* __restrict__ logits, int* __restrict__ ids,
                                                        int B, int T, int steps, int n_class) {
  __shared__ __attribute__((aligned(16))) float hs[16 * M_HP];
  __shared__ __attribute__((aligned(16))) float cs[16 * M_HP];
  __shared__ __attribute__((aligned(16))) float ps[16 * M_HP];
  __shared__ float lg[16][M_MAXCLS + 1];
  __shared__ int ys[16];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int b0 = blockIdx.x * 16;
  const int ar = lane & 15, ak = 4 * (lane >> 4);        // this lane's operand row and k offset inside a 16-wide chunk
  const int col = 16 * q + ar;                           // the output column of this lane in phases 1 and 3
  for (int i = tid; i < 16 * M_HP; i += 1024) hs[i] = 0.f;
  if (tid < 16) ys[tid] = 0;
  __syncthreads();
  const int bq = min(b0 + q, B - 1);                     // phase 2: the image of this wave (tiles past B repeat the last image)
  const float4 sw = *reinterpret_cast<const float4*>(w.score_w + 4 * lane);
  const float h2h_b = w.h2h_b[col];
  const float bh_r = w.bhh[col], bh_z = w.bhh[MH + col], bh_n = w.bhh[2 * MH + col];
  for (int s = 0; s < steps; ++s) {
    {
      const f32x4 acc = tile_k256(&hs[ar * M_HP + ak], w.h2h_w + (size_t)col * MH + ak);
#pragma unroll
      for (int r = 0; r < 4; ++r) ps[((lane >> 4) * 4 + r) * M_HP + col] = acc[r] + h2h_b;
    }
    __syncthreads();
    {
      const float4 hp = *reinterpret_cast<const float4*>(&ps[q * M_HP + 4 * lane]);
      float e = -INFINITY;
      for (int t = 0; t < T; ++t) {
        const float4 xp = *reinterpret_cast<const float4*>(fproj + ((size_t)bq * T + t) * MH + 4 * lane);
        float a = (sw.x * tanhf(xp.x + hp.x) + sw.y * tanhf(xp.y + hp.y)) + (sw.z * tanhf(xp.z + hp.z) + sw.w * tanhf(xp.w + hp.w));
        a = wave_sum(a);
        if (lane == t) e = a;
      }
      const float m = wave_max(e);
      const float pe = lane < T ? expf(e - m) : 0.f;
      const float alpha = pe / wave_sum(pe);
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = 0; t < T; ++t) {
        const float al = __shfl(alpha, t, 64);
        const float4 f = *reinterpret_cast<const float4*>(feats + ((size_t)bq * T + t) * MH + 4 * lane);
        c.x += al * f.x; c.y += al * f.y; c.z += al * f.z; c.w += al * f.w;
      }
      *reinterpret_cast<float4*>(&cs[q * M_HP + 4 * lane]) = c;
    }
    __syncthreads();
    float hn[4];
    {
      const float* ca = &cs[ar * M_HP + ak];
      const float* ha = &hs[ar * M_HP + ak];
      const f32x4 ir = tile_k256(ca, w.wih_ctx + (size_t)col * MH + ak);
      const f32x4 iz = tile_k256(ca, w.wih_ctx + (size_t)(MH + col) * MH + ak);
      const f32x4 in = tile_k256(ca, w.wih_ctx + (size_t)(2 * MH + col) * MH + ak);
      const f32x4 hr = tile_k256(ha, w.whh + (size_t)col * MH + ak);
      const f32x4 hz = tile_k256(ha, w.whh + (size_t)(MH + col) * MH + ak);
      const f32x4 hh = tile_k256(ha, w.whh + (size_t)(2 * MH + col) * MH + ak);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;
        const float* e = w.E + (size_t)ys[row] * MG + col;
        const float r_ = sigmoid_f((e[0] + ir[r]) + (hr[r] + bh_r)), z_ = sigmoid_f((e[MH] + iz[r]) + (hz[r] + bh_z));
        const float n_ = tanhf((e[2 * MH] + in[r]) + r_ * (hh[r] + bh_n));
        hn[r] = (1.0f - z_) * n_ + z_ * hs[row * M_HP + col];
      }
    }
    __syncthreads();                                     // every wave has read the old state
#pragma unroll
    for (int r = 0; r < 4; ++r) hs[((lane >> 4) * 4 + r) * M_HP + col] = hn[r];
    __syncthreads();
    if (16 * q < n_class) {
      const int c = min(col, n_class - 1);
      const f32x4 acc = tile_k256(&hs[ar * M_HP + ak], w.gen_w + (size_t)c * MH + ak);
      const float gb = w.gen_b[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;
        const float v = acc[r] + gb;
        lg[row][col] = v;
        if (col < n_class && b0 + row < B) logits[((size_t)(b0 + row) * steps + s) * n_class + col] = v;
      }
    }
    __syncthreads();
    if (tid < 16) {
      int best = 0;
      float bv = lg[tid][0];
      for (int c = 1; c < n_class; ++c)
        if (lg[tid][c] > bv) { bv = lg[tid][c]; best = c; }       // equal logits: the lower class index
      ys[tid] = best + 1;
      if (b0 + tid < B) ids[(size_t)(b0 + tid) * steps + s] = best;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int dpmn_moran_rectify_f32(const float* omap, const float* plane, const float* grid_x, const float* grid_y, const float* acc_in,
                           float* acc_out, float* rect, float* rect_nhwc4, int B, int H, int W, int Hm, int Wm, dpmn_stream_t stream) {
  DPMN_REQUIRE(omap && plane && grid_x && grid_y && acc_out && rect && rect_nhwc4, "moran_rectify: null pointer");
  DPMN_REQUIRE(B > 0 && H > 0 && W > 0 && Hm > 1 && Wm > 1, "moran_rectify: the offset map must be at least 2 x 2 (MaxPool2d(2, 1))");
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(k_moran_rectify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), omap, plane, grid_x, grid_y, acc_in,
                     acc_out, rect, rect_nhwc4, B, H, W, Hm, Wm);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_moran_split_nhwc_f32(const float* x, float* y1, float* y2, int B, int H, int W, int C, int sy, int sx, dpmn_stream_t stream) {
  DPMN_REQUIRE(x && y1 && y2 && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && sy > 0 && sx > 0,
               "moran_split_nhwc: NHWC with 2 C channels, C % 4 == 0, strides > 0");
  const int Ho = (H - 1) / sy + 1, Wo = (W - 1) / sx + 1;
  const long n = (long)B * Ho * Wo * (C / 2);
  hipLaunchKernelGGL(k_moran_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, y1, y2, B, H, W, C, sy, sx, Ho, Wo);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_moran_decode_f32(const dpmn_moran_dec_weights* w, const float* feats, const float* fproj, float* logits, int* ids, int B, int T,
                          int steps, int n_class, dpmn_stream_t stream) {
  DPMN_REQUIRE(w && w->h2h_w && w->h2h_b && w->score_w && w->E && w->wih_ctx && w->whh && w->bhh && w->gen_w && w->gen_b && feats && fproj &&
                   logits && ids,
               "moran_decode: null pointer");
  DPMN_REQUIRE(B > 0 && T > 0 && T <= M_MAXT && steps > 0 && n_class > 0 && n_class <= M_MAXCLS, "moran_decode: 1..64 positions, 1..48 classes");
  hipLaunchKernelGGL(k_moran_decode, dim3((unsigned)cdiv(B, 16)), dim3(1024), 0, as_stream(stream), feats, fproj, *w, logits, ids, B, T, steps,
                     n_class);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
