// Kernels of the native CRNN recogniser (model/crnn.py NativeCRNN; reference model/crnn/crnn.py) that are not a conv / GEMM:
//   k_gray_prep       parse_crnn_data (base.py:419-425): torch's bicubic resize to Ho x Wo + ITU-601 luma, NHWC with 4 channels
//                     (parse_moran_data is the same arithmetic; NativeMORAN also takes the luma as a plane)
//   k_maxpool2d       nn.MaxPool2d(k, stride, padding) over NHWC with -inf padding (pooling2 / pooling3: (2,2), (2,1), (0,1))
//   k_lstm_step       one time step of a bidirectional nn.LSTM, both directions and the whole batch in one launch: h W_hh^T on
//                     fp32 MFMA with the cell update in the epilogue
//   k_ctc_greedy      strLabelConverter.decode(raw=False) (utils_crnn.py:54-90) after the arg-max: collapse repeats, drop blank 0
//   k_crnn_label_vecs CRNN.label_vecs: softmax over the classes, (B, T, n_class) rows -> (B, n_class, 1, T)
#include "common.h"

namespace {

// get_cubic_upsample_coefficients (ATen UpSample.h), A = -0.75
__device__ __forceinline__ void cubic_coeffs(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float x1 = t + 1.0f, x2 = 1.0f - t, x3 = x2 + 1.0f;
  w[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
  w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

// source index (dst + 0.5) * in / out - 0.5 (not clamped), base index min(floor, in - 1), fraction clamped to [0, 1]
// (area_pixel_compute_source_index + guard_index_and_lambda)
__device__ __forceinline__ int cubic_src(int dst, int in, int out, float& t) {
  const float scale = (float)in / (float)out;
  const float real = scale * ((float)dst + 0.5f) - 0.5f;
  const int i0 = min((int)floorf(real), in - 1);
  t = fminf(fmaxf(real - (float)i0, 0.0f), 1.0f);
  return i0;
}

// one output pixel per thread: out[b][y][x] = (luma, 0, 0, 0); luma = 0.299 R + 0.587 G + 0.114 B of the bicubic samples; plane
// (optional): the same luma as a (B, Ho, Wo) plane (parse_moran_data: the image MORN's warp samples)
__global__ void k_gray_prep(const float* __restrict__ img, long img_stride, float* __restrict__ out, float* __restrict__ plane, int B, int H,
                            int W, int Ho, int Wo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * Ho * Wo) return;
  const int x = idx % Wo, y = (idx / Wo) % Ho, b = idx / ((long)Wo * Ho);
  float ty, tx, wy[4], wx[4];
  const int y0 = cubic_src(y, H, Ho, ty), x0 = cubic_src(x, W, Wo, tx);
  cubic_coeffs(ty, wy);
  cubic_coeffs(tx, wx);
  int ys[4], xs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ys[i] = min(max(y0 - 1 + i, 0), H - 1);
    xs[i] = min(max(x0 - 1 + i, 0), W - 1);
  }
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = img + (size_t)b * img_stride + (size_t)c * H * W;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {       // rows outer, columns inner (the order of ATen's separable cubic interpolation)
      const float* r = p + (size_t)ys[i] * W;
      const float row = ((r[xs[0]] * wx[0] + r[xs[1]] * wx[1]) + r[xs[2]] * wx[2]) + r[xs[3]] * wx[3];
      acc = i == 0 ? row * wy[0] : acc + row * wy[i];
    }
    v[c] = acc;
  }
  const float luma = (0.299f * v[0] + 0.587f * v[1]) + 0.114f * v[2];
  *reinterpret_cast<float4*>(out + idx * 4) = make_float4(luma, 0.f, 0.f, 0.f);
  if (plane) plane[idx] = luma;
}

// one float4 of output channels per thread; window taps outside the plane are -inf (skipped)
__global__ void k_maxpool2d(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C, int kh, int kw, int sh,
                            int sw, int ph, int pw, int Ho, int Wo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 4;
  if (idx >= (long)B * Ho * Wo * C4) return;
  const int c4 = idx % C4;
  const long p = idx / C4;
  const int ox = p % Wo, oy = (p / Wo) % Ho, b = p / ((long)Wo * Ho);
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int ky = 0; ky < kh; ++ky) {
    const int iy = oy * sh - ph + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < kw; ++kx) {
      const int ix = ox * sw - pw + kx;
      if (ix < 0 || ix >= W) continue;
      const float4 v = *reinterpret_cast<const float4*>(x + (((size_t)b * H + iy) * W + ix) * C + c4 * 4);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  }
  *reinterpret_cast<float4*>(y + (size_t)idx * 4) = m;
}

// Step s of both directions (forward: t = s, backward: t = T-1-s), torch's gate order i, f, g, o; h0 = c0 = 0.
//   gx   (B*T, 8*HID): x W_ih^T + b_ih + b_hh, row b*T + t, columns [forward i f g o | backward i f g o]
//   whh  (2, 4*HID, HID): W_hh of the forward and backward direction
//   out  (B*T, 2*HID): [h_fwd | h_bwd] per row; h of the previous step is read from here
//   cst  (2, B, HID): cell state, updated in place (every element has exactly one owner thread)
// Block = 16 hidden units x 16 images, 4 waves: wave q computes gate q's 16 x 16 tile of h W_hh^T with v_mfma_f32_16x16x4_f32
// (A = h rows from LDS, B = W_hh rows from L2), the tiles meet in LDS, and one thread per (image, unit) applies the cell update.
template <int HID>
__global__ __launch_bounds__(256) void k_lstm_step(const float* __restrict__ gx, const float* __restrict__ whh, float* __restrict__ out,
                                                    float* __restrict__ cst, int B, int T, int s) {
  static_assert(HID % 16 == 0, "hidden size: whole 16-unit slices");
  constexpr int HP = HID + 4;         // LDS row pitch: the 16 rows of a 16-lane group start 4 banks apart
  __shared__ __attribute__((aligned(16))) float hs[16 * HP];
  __shared__ float gs[4][16][17];
  const int j0 = blockIdx.x * 16, d = blockIdx.y, b0 = blockIdx.z * 16;
  const int t = d == 0 ? s : T - 1 - s;
  const int tp = d == 0 ? t - 1 : t + 1;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  for (int e = tid; e < 16 * (HID / 4); e += 256) {
    const int r = e / (HID / 4), c4 = e - r * (HID / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s > 0 && b0 + r < B) v = *reinterpret_cast<const float4*>(out + ((size_t)(b0 + r) * T + tp) * (2 * HID) + d * HID + c4 * 4);
    *reinterpret_cast<float4*>(&hs[r * HP + c4 * 4]) = v;
  }
  __syncthreads();
  // lane l holds k = 4 (l >> 4) .. +3 of every 16-wide k chunk for row l & 15 of both operands: the four MFMAs of a chunk walk the
  // float4 element by element (the k order inside a chunk is a permutation, the same on both sides)
  const float* wr = whh + ((size_t)(d * 4 + q) * HID + j0 + (lane & 15)) * HID + 4 * (lane >> 4);
  const float* hr = &hs[(lane & 15) * HP + 4 * (lane >> 4)];
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < HID; k += 16) {
    const float4 w = *reinterpret_cast<const float4*>(wr + k);
    const float4 h = *reinterpret_cast<const float4*>(hr + k);
    acc0 = mfma16(h.x, w.x, acc0);
    acc1 = mfma16(h.y, w.y, acc1);
    acc0 = mfma16(h.z, w.z, acc0);
    acc1 = mfma16(h.w, w.w, acc1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) gs[q][(lane >> 4) * 4 + r][lane & 15] = acc0[r] + acc1[r];
  __syncthreads();
  const int bl = tid >> 4, j = tid & 15, b = b0 + bl;
  if (b >= B) return;
  const size_t row = (size_t)b * T + t;
  const float* g = gx + row * (8 * HID) + d * 4 * HID + j0 + j;
  const float gi = g[0] + gs[0][bl][j], gf = g[HID] + gs[1][bl][j], gg = g[2 * HID] + gs[2][bl][j], go = g[3 * HID] + gs[3][bl][j];
  const float i_ = sigmoid_f(gi), f_ = sigmoid_f(gf), g_ = tanhf(gg), o_ = sigmoid_f(go);
  float* cp = cst + ((size_t)d * B + b) * HID + j0 + j;
  const float c = s > 0 ? f_ * *cp + i_ * g_ : i_ * g_;
  *cp = c;
  out[row * (2 * HID) + d * HID + j0 + j] = o_ * tanhf(c);
}

// one thread per image: cls[b][0 .. length) = the arg-max classes (first maximum) of rows b*T + t with repeats collapsed and
// blanks (class 0) dropped, cls[b][length .. T) = 0
__global__ void k_ctc_greedy(const float* __restrict__ logits, int ld, int n_class, int* __restrict__ cls, int* __restrict__ length,
                             int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int n = 0, prev = -1;
  for (int t = 0; t < T; ++t) {
    const float* r = logits + ((size_t)b * T + t) * ld;
    int best = 0;
    float bv = r[0];
    for (int c = 1; c < n_class; ++c)
      if (r[c] > bv) { bv = r[c]; best = c; }
    if (best != 0 && best != prev) cls[(size_t)b * T + n++] = best;
    prev = best;
  }
  length[b] = n;
  for (int t = n; t < T; ++t) cls[(size_t)b * T + t] = 0;
}

// one thread per (image, step): softmax over n_class logits of row b*T + t -> out[b][c][0][t]
__global__ void k_crnn_label_vecs(const float* __restrict__ logits, int ld, int n_class, float* __restrict__ out, int B, int T) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * T) return;
  const int b = idx / T, t = idx - b * T;
  const float* r = logits + (size_t)idx * ld;
  float m = r[0];
  for (int c = 1; c < n_class; ++c) m = fmaxf(m, r[c]);
  float sum = 0.f;
  for (int c = 0; c < n_class; ++c) sum += expf(r[c] - m);
  float* o = out + (size_t)b * n_class * T + t;
  for (int c = 0; c < n_class; ++c) o[(size_t)c * T] = expf(r[c] - m) / sum;
}

}  // namespace

extern "C" {

int dpmn_gray_prep_f32(const float* img, long img_stride, float* plane, float* out_nhwc4, int B, int H, int W, int Ho, int Wo,
                       dpmn_stream_t stream) {
  DPMN_REQUIRE(img && out_nhwc4 && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && img_stride >= 3L * H * W, "gray_prep: bad arguments");
  const long n = (long)B * Ho * Wo;
  hipLaunchKernelGGL(k_gray_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), img, img_stride, out_nhwc4, plane, B, H,
                     W, Ho, Wo);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_maxpool2d_f32(const float* x, float* y, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                       dpmn_stream_t stream) {
  DPMN_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "maxpool2d: NHWC with C % 4 == 0");
  DPMN_REQUIRE(kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0 && 2 * ph <= kh && 2 * pw <= kw,
               "maxpool2d: padding at most half the window (nn.MaxPool2d's rule)");
  const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
  DPMN_REQUIRE(Ho > 0 && Wo > 0, "maxpool2d: window larger than the padded plane");
  const long n = (long)B * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(k_maxpool2d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, B, H, W, C, kh, kw, sh, sw, ph,
                     pw, Ho, Wo);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_bilstm_f32(const float* gx, const float* w_hh, float* out, float* c_state, int B, int T, int H, dpmn_stream_t stream) {
  DPMN_REQUIRE(gx && w_hh && out && c_state && B > 0 && T > 0, "bilstm: bad arguments");
  DPMN_REQUIRE(H == 256, "bilstm: built for hidden size 256 (CRNN's BidirectionalLSTM)");
  const dim3 grid(H / 16, 2, (unsigned)cdiv(B, 16));
  for (int s = 0; s < T; ++s) {
    hipLaunchKernelGGL(k_lstm_step<256>, grid, dim3(256), 0, as_stream(stream), gx, w_hh, out, c_state, B, T, s);
    DPMN_CHECK_LAUNCH();
  }
  return DPMN_OK;
}

int dpmn_ctc_greedy_i32(const float* logits, int ld, int n_class, int* cls, int* length, int B, int T, dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && cls && length && B > 0 && T > 0 && n_class > 0 && ld >= n_class, "ctc_greedy: bad arguments");
  hipLaunchKernelGGL(k_ctc_greedy, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, as_stream(stream), logits, ld, n_class, cls, length, B, T);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_crnn_label_vecs_f32(const float* logits, int ld, int n_class, float* out, int B, int T, dpmn_stream_t stream) {
  DPMN_REQUIRE(logits && out && B > 0 && T > 0 && n_class > 0 && ld >= n_class, "crnn_label_vecs: bad arguments");
  hipLaunchKernelGGL(k_crnn_label_vecs, dim3((unsigned)cdiv(B * T, 256)), dim3(256), 0, as_stream(stream), logits, ld, n_class, out, B, T);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
