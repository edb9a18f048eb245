// Kernels of the native ASTER recogniser (model/aster.py NativeASTER; reference model/recognizer/) that are not a conv / GEMM /
// pool / BiLSTM:
//   k_aster_prep      parse_aster_data (x * 2 - 1) + F.interpolate(x, (32, 64), bilinear, align_corners=True): one launch writes the
//                     normalised NCHW image (the TPS source) and the NHWC(4) input of the STN head
//   k_subsample_nhwc  y[b][oy][ox] = x[b][oy * sy][ox * sx]: the row / column gather in front of a strided 1 x 1 conv (ResNet_ASTER's
//                     (2, 1) downsampling convs; dpmn_conv_desc has one scalar stride)
// and the attention decoder with beam search (attention_recognition_head.py:68-122, 187-268), four launches per step:
//   k_dec_sproj       sProj = sEmbed(s) for all beam rows, fp32 MFMA
//   k_dec_attend      e_t = w . tanh(sProj + xProj[img, t]) + b, softmax over t, context = alpha . feats[img]
//   k_dec_gru         GRU cell: context W_ih[:, 512:]^T and s W_hh^T on fp32 MFMA, the embedding half of the input product as a row
//                     of the precomputed table E = tgt_embedding W_ih[:, :512]^T + b_ih, torch's gate formula in the epilogue
//   k_dec_topk        per image: fc + log-softmax of its beams, sequence scores, top `beam` of beam x n_class candidates (ties: the
//                     lower flat index wins), step record, EOS erase, state reorder by predecessor
// The decoder stays on v_mfma_f32_16x16x4_f32 in every compute mode.  The state is double-buffered: k_dec_gru reads `state` and
// writes `snew`, k_dec_topk reads `snew` and writes `state`.
#include "common.h"

namespace {

constexpr int AD = 512;           // sDim = attDim = xDim = emdDim
constexpr int AG = 3 * AD;        // GRU gate rows (r, z, n)
constexpr int A_MAXT = 64;        // encoder positions (25 for 32 x 100 rectified images)
constexpr int A_MAXBEAM = 8;
constexpr int A_MAXCLS = 128;

// area_pixel_compute_source_index with align_corners=True: src = dst * (in - 1) / (out - 1)
__device__ __forceinline__ int lin_src(int dst, int in, int out, float& l1) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
  const float real = scale * (float)dst;
  const int i0 = min((int)real, in - 1);
  l1 = real - (float)i0;
  return i0;
}

__global__ void k_aster_prep(const float* __restrict__ img, long img_stride, float* __restrict__ norm, float* __restrict__ stn, int B,
                             int H, int W, int Hs, int Ws) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n_img = (long)B * 3 * H * W;
  if (idx < n_img) {
    const long hw = (long)H * W;
    const int b = idx / (3 * hw);
    const long r = idx - (long)b * 3 * hw;
    norm[idx] = img[(size_t)b * img_stride + r] * 2.0f - 1.0f;
  }
  if (idx < (long)B * Hs * Ws) {
    const int x = idx % Ws, y = (idx / Ws) % Hs, b = idx / ((long)Ws * Hs);
    float ly, lx;
    const int y0 = lin_src(y, H, Hs, ly), x0 = lin_src(x, W, Ws, lx);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = img + (size_t)b * img_stride + (size_t)c * H * W;
      const float v00 = p[(size_t)y0 * W + x0] * 2.0f - 1.0f, v01 = p[(size_t)y0 * W + x1] * 2.0f - 1.0f;
      const float v10 = p[(size_t)y1 * W + x0] * 2.0f - 1.0f, v11 = p[(size_t)y1 * W + x1] * 2.0f - 1.0f;
      v[c] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);      // upsample_bilinear2d's grouping
    }
    *reinterpret_cast<float4*>(stn + idx * 4) = make_float4(v[0], v[1], v[2], 0.f);
  }
}

__global__ void k_subsample_nhwc(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C, int sy, int sx, int Ho,
                                 int Wo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 4;
  if (idx >= (long)B * Ho * Wo * C4) return;
  const int c4 = idx % C4;
  const long p = idx / C4;
  const int ox = p % Wo, oy = (p / Wo) % Ho, b = p / ((long)Wo * Ho);
  *reinterpret_cast<float4*>(y + (size_t)idx * 4) =
      *reinterpret_cast<const float4*>(x + (((size_t)b * H + (size_t)oy * sy) * W + (size_t)ox * sx) * C + (size_t)c4 * 4);
}

// 16 x 16 tile of A W^T over K = 512: a / w point at this lane's row of each operand, already advanced by 4 (lane >> 4) floats; the four
// MFMAs of a 16-wide k chunk walk the float4 element by element (the k order inside a chunk is the same permutation on both sides)
__device__ __forceinline__ f32x4 tile_k512(const float* __restrict__ a, const float* __restrict__ w) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int k = 0; k < AD; k += 16) {
    const float4 av = *reinterpret_cast<const float4*>(a + k);
    const float4 wv = *reinterpret_cast<const float4*>(w + k);
    acc0 = mfma16(av.x, wv.x, acc0);
    acc1 = mfma16(av.y, wv.y, acc1);
    acc0 = mfma16(av.z, wv.z, acc0);
    acc1 = mfma16(av.w, wv.w, acc1);
  }
  return acc0 + acc1;
}

// sproj (R, 512) = state (R, 512) sEmbed^T + b.  Block = 16 rows x 64 columns, wave q owns 16 columns.  Rows past R read row R - 1
// and are not stored.
__global__ __launch_bounds__(256) void k_dec_sproj(const float* __restrict__ state, const float* __restrict__ sw, const float* __restrict__ sb,
                                                    float* __restrict__ sproj, int R) {
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 16, j0 = blockIdx.x * 64 + q * 16;
  const int ar = min(r0 + (lane & 15), R - 1);
  const f32x4 acc = tile_k512(state + (size_t)ar * AD + 4 * (lane >> 4), sw + (size_t)(j0 + (lane & 15)) * AD + 4 * (lane >> 4));
  const int col = j0 + (lane & 15);
  const float bias = sb[col];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + (lane >> 4) * 4 + r;
    if (row < R) sproj[(size_t)row * AD + col] = acc[r] + bias;
  }
}

// one block per beam row; image of the row = row_img[row] or row / beam
__global__ __launch_bounds__(256) void k_dec_attend(const float* __restrict__ sproj, const float* __restrict__ xproj,
                                                     const float* __restrict__ feats, const float* __restrict__ ww, const float* __restrict__ wb,
                                                     const int* __restrict__ row_img, int beam, float* __restrict__ ctx,
                                                     float* __restrict__ alpha_out, int T) {
  __shared__ float e_s[A_MAXT];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int b = row_img ? row_img[row] : row / beam;
  float sp[8], wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sp[i] = sproj[(size_t)row * AD + lane + 64 * i];
    wv[i] = ww[lane + 64 * i];
  }
  for (int t = q; t < T; t += 4) {
    const float* xp = xproj + ((size_t)b * T + t) * AD;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) a += wv[i] * tanhf(sp[i] + xp[lane + 64 * i]);
    a = wave_sum(a);
    if (lane == 0) e_s[t] = a + wb[0];
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = 0; t < T; ++t) m = fmaxf(m, e_s[t]);
  float sum = 0.f;
  for (int t = 0; t < T; ++t) sum += expf(e_s[t] - m);
  const float inv = 1.0f / sum;
  float c0 = 0.f, c1 = 0.f;
  for (int t = 0; t < T; ++t) {
    const float al = expf(e_s[t] - m) * inv;
    const float* f = feats + ((size_t)b * T + t) * AD;
    c0 += al * f[tid];
    c1 += al * f[tid + 256];
  }
  ctx[(size_t)row * AD + tid] = c0;
  ctx[(size_t)row * AD + tid + 256] = c1;
  if (alpha_out && tid < T) alpha_out[(size_t)row * T + tid] = expf(e_s[tid] - m) * inv;
}

// Block = 16 hidden units x 16 rows, 6 waves: waves 0..2 the (r, z, n) tiles of ctx W_ih[:, 512:]^T, waves 3..5 of state W_hh^T; then
// one thread per (row, unit): r = sig(i_r + h_r), z = sig(i_z + h_z), n = tanh(i_n + r (h_n + b_hn)), s' = (1 - z) n + z s with
// i = E[y_prev] + ctx part (b_ih is inside E) and h = state part + b_hh
__global__ __launch_bounds__(384) void k_dec_gru(const float* __restrict__ ctx, const float* __restrict__ state, const int* __restrict__ yprev,
                                                  const float* __restrict__ E, const float* __restrict__ wih_ctx, const float* __restrict__ whh,
                                                  const float* __restrict__ bhh, float* __restrict__ snew, int R) {
  __shared__ float gs[6][16][17];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int j0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const int ar = min(r0 + (lane & 15), R - 1);
  const float* a = (q < 3 ? ctx : state) + (size_t)ar * AD + 4 * (lane >> 4);
  const float* w = (q < 3 ? wih_ctx : whh) + ((size_t)(q % 3) * AD + j0 + (lane & 15)) * AD + 4 * (lane >> 4);
  const f32x4 acc = tile_k512(a, w);
#pragma unroll
  for (int r = 0; r < 4; ++r) gs[q][(lane >> 4) * 4 + r][lane & 15] = acc[r];
  __syncthreads();
  if (tid >= 256) return;
  const int bl = tid >> 4, j = tid & 15, row = r0 + bl, col = j0 + j;
  if (row >= R) return;
  const float* e = E + (size_t)yprev[row] * AG + col;
  const float ir = e[0] + gs[0][bl][j], iz = e[AD] + gs[1][bl][j], in = e[2 * AD] + gs[2][bl][j];
  const float hr = gs[3][bl][j] + bhh[col], hz = gs[4][bl][j] + bhh[AD + col], hn = gs[5][bl][j] + bhh[2 * AD + col];
  const float r_ = sigmoid_f(ir + hr), z_ = sigmoid_f(iz + hz);
  const float n_ = tanhf(in + r_ * hn);
  snew[(size_t)row * AD + col] = (1.0f - z_) * n_ + z_ * state[(size_t)row * AD + col];
}

__device__ __forceinline__ float dot512(const float* __restrict__ w, const float* s) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = 0; k < AD; k += 4) {
    const float4 wv = *reinterpret_cast<const float4*>(w + k);
    const float4 sv = *reinterpret_cast<const float4*>(s + k);
    a0 += wv.x * sv.x; a1 += wv.y * sv.y; a2 += wv.z * sv.z; a3 += wv.w * sv.w;
  }
  return (a0 + a1) + (a2 + a3);
}

// logits (R, n_class) = fc(s): the classifier of one teacher-forced step (decode_step)
__global__ __launch_bounds__(128) void k_dec_fc(const float* __restrict__ s, const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                 float* __restrict__ logits, int n_class) {
  __shared__ __attribute__((aligned(16))) float ss[AD];
  const int row = blockIdx.x;
  for (int i = threadIdx.x; i < AD; i += 128) ss[i] = s[(size_t)row * AD + i];
  __syncthreads();
  for (int c = threadIdx.x; c < n_class; c += 128) logits[(size_t)row * n_class + c] = dot512(fcw + (size_t)c * AD, ss) + fcb[c];
}

__global__ void k_beam_init(float* __restrict__ state, float* __restrict__ seq, int* __restrict__ yprev, int R, int beam, int bos) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < R * AD) state[idx] = 0.f;
  if (idx < R) {
    seq[idx] = idx % beam == 0 ? 0.f : -INFINITY;
    yprev[idx] = bos;
  }
}

// one block per image, 512 threads
__global__ __launch_bounds__(512) void k_dec_topk(const float* __restrict__ snew, const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                   float* __restrict__ seq, int* __restrict__ yprev, float* __restrict__ state,
                                                   int* __restrict__ sym, int* __restrict__ pred, float* __restrict__ score, int beam, int n_class,
                                                   int eos) {
  __shared__ __attribute__((aligned(16))) float ss[A_MAXBEAM * AD];
  __shared__ float cand[A_MAXBEAM * A_MAXCLS];
  __shared__ float lse[A_MAXBEAM];
  __shared__ int sel[A_MAXBEAM];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int row0 = b * beam, n_cand = beam * n_class;
  for (int i = tid; i < beam * AD; i += 512) ss[i] = snew[(size_t)row0 * AD + i];
  __syncthreads();
  for (int i = tid; i < n_cand; i += 512) {
    const int k = i / n_class, c = i - k * n_class;
    cand[k * A_MAXCLS + c] = dot512(fcw + (size_t)c * AD, ss + k * AD) + fcb[c];
  }
  __syncthreads();
  for (int k = q; k < beam; k += 8) {       // log-softmax of beam k: x - max - log(sum exp(x - max))
    float m = -INFINITY;
    for (int c = lane; c < n_class; c += 64) m = fmaxf(m, cand[k * A_MAXCLS + c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < n_class; c += 64) s += expf(cand[k * A_MAXCLS + c] - m);
    s = wave_sum(s);
    if (lane == 0) lse[k] = m + logf(s);
  }
  __syncthreads();
  for (int i = tid; i < n_cand; i += 512) {
    const int k = i / n_class, c = i - k * n_class;
    cand[k * A_MAXCLS + c] = seq[row0 + k] + (cand[k * A_MAXCLS + c] - lse[k]);
  }
  __syncthreads();
  if (q == 0) {       // top `beam` of the candidates, best first; equal scores: the lower flat index beam * n_class + class
    int chosen[A_MAXBEAM];      // every lane holds the same list (the butterfly leaves the winner in all lanes)
#pragma unroll
    for (int sidx = 0; sidx < A_MAXBEAM; ++sidx) {
      chosen[sidx] = -1;
      if (sidx < beam) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = lane; i < n_cand; i += 64) {
          const int k = i / n_class, c = i - k * n_class;
          const float v = cand[k * A_MAXCLS + c];
          bool taken = v != v;                  // a NaN never wins
#pragma unroll
          for (int p = 0; p < sidx; ++p) taken |= chosen[p] == i;
          if (!taken && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = xshfl_v(bv, o);
          const int oi = xshfl_v(bi, o);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi == 0x7fffffff) bi = sidx;        // only NaNs left: keep the indices valid
        chosen[sidx] = bi;
        if (lane == 0) sel[sidx] = bi;
      }
    }
  }
  __syncthreads();
  if (tid < beam) {
    const int i = sel[tid], k = i / n_class, c = i - k * n_class;
    const float v = cand[k * A_MAXCLS + c];
    sym[row0 + tid] = c;
    pred[row0 + tid] = row0 + k;
    score[row0 + tid] = v;
    yprev[row0 + tid] = c;
    seq[row0 + tid] = c == eos ? -INFINITY : v;
  }
  for (int i = tid; i < beam * AD; i += 512) {
    const int k = i / AD, d = i - k * AD;
    state[(size_t)row0 * AD + i] = ss[(sel[k] / n_class) * AD + d];
  }
}

int check_weights(const dpmn_aster_dec_weights* w) {
  return w && w->s_w && w->s_b && w->w_w && w->w_b && w->E && w->wih_ctx && w->whh && w->bhh && w->fc_w && w->fc_b;
}

}  // namespace

extern "C" {

int dpmn_aster_prep_f32(const float* img, long img_stride, float* norm_nchw, float* stn_nhwc4, int B, int H, int W, int Hs, int Ws,
                        dpmn_stream_t stream) {
  DPMN_REQUIRE(img && norm_nchw && stn_nhwc4 && B > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0 && img_stride >= 3L * H * W,
               "aster_prep: bad arguments");
  const long n = (long)B * 3 * H * W > (long)B * Hs * Ws ? (long)B * 3 * H * W : (long)B * Hs * Ws;
  hipLaunchKernelGGL(k_aster_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), img, img_stride, norm_nchw, stn_nhwc4,
                     B, H, W, Hs, Ws);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_subsample_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, int sy, int sx, dpmn_stream_t stream) {
  DPMN_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && sy > 0 && sx > 0, "subsample_nhwc: NHWC with C % 4 == 0, strides > 0");
  const int Ho = (H - 1) / sy + 1, Wo = (W - 1) / sx + 1;
  const long n = (long)B * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(k_subsample_nhwc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, B, H, W, C, sy, sx, Ho, Wo);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

size_t dpmn_aster_beam_workspace_bytes(int B, int beam) {
  const size_t R = (size_t)B * beam;
  return (4 * R * AD + 2 * R) * sizeof(float);
}

int dpmn_aster_decode_step_f32(const dpmn_aster_dec_weights* w, const float* feats, const float* xproj, const int* row_img,
                               const float* state, const int* y_prev, float* sproj, float* ctx, float* alpha, float* state_out,
                               float* logits, int R, int T, int n_class, dpmn_stream_t stream) {
  DPMN_REQUIRE(check_weights(w) && feats && xproj && row_img && state && y_prev && sproj && ctx && alpha && state_out && logits,
               "aster_decode_step: null pointer");
  DPMN_REQUIRE(R > 0 && T > 0 && T <= A_MAXT && n_class > 0 && n_class <= A_MAXCLS, "aster_decode_step: 1..64 positions, 1..128 classes");
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_dec_sproj, dim3(AD / 64, cdiv(R, 16)), dim3(256), 0, st, state, w->s_w, w->s_b, sproj, R);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dec_attend, dim3(R), dim3(256), 0, st, sproj, xproj, feats, w->w_w, w->w_b, row_img, 1, ctx, alpha, T);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dec_gru, dim3(AD / 16, cdiv(R, 16)), dim3(384), 0, st, ctx, state, y_prev, w->E, w->wih_ctx, w->whh, w->bhh,
                     state_out, R);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dec_fc, dim3(R), dim3(128), 0, st, state_out, w->fc_w, w->fc_b, logits, n_class);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_aster_beam_f32(const dpmn_aster_dec_weights* w, const float* feats, const float* xproj, float* ws, size_t ws_bytes, int* sym,
                        int* pred, float* score, int B, int T, int beam, int n_class, int eos, int steps, dpmn_stream_t stream) {
  DPMN_REQUIRE(check_weights(w) && feats && xproj && ws && sym && pred && score, "aster_beam: null pointer");
  DPMN_REQUIRE(B > 0 && T > 0 && T <= A_MAXT && beam > 0 && beam <= A_MAXBEAM && n_class >= beam && n_class <= A_MAXCLS && steps > 0 &&
                   eos >= 0 && eos < n_class,
               "aster_beam: 1..64 positions, beam 1..8, beam..128 classes");
  DPMN_REQUIRE(ws_bytes >= dpmn_aster_beam_workspace_bytes(B, beam), "aster_beam: workspace too small");
  const int R = B * beam;
  float* state = ws;
  float* snew = state + (size_t)R * AD;
  float* sproj = snew + (size_t)R * AD;
  float* ctx = sproj + (size_t)R * AD;
  float* seq = ctx + (size_t)R * AD;
  int* yprev = reinterpret_cast<int*>(seq + R);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_beam_init, dim3(cdiv(R * AD, 256)), dim3(256), 0, st, state, seq, yprev, R, beam, n_class);
  DPMN_CHECK_LAUNCH();
  for (int i = 0; i < steps; ++i) {
    hipLaunchKernelGGL(k_dec_sproj, dim3(AD / 64, cdiv(R, 16)), dim3(256), 0, st, state, w->s_w, w->s_b, sproj, R);
    hipLaunchKernelGGL(k_dec_attend, dim3(R), dim3(256), 0, st, sproj, xproj, feats, w->w_w, w->w_b, (const int*)nullptr, beam, ctx,
                       (float*)nullptr, T);
    hipLaunchKernelGGL(k_dec_gru, dim3(AD / 16, cdiv(R, 16)), dim3(384), 0, st, ctx, state, yprev, w->E, w->wih_ctx, w->whh, w->bhh, snew, R);
    hipLaunchKernelGGL(k_dec_topk, dim3(B), dim3(512), 0, st, snew, w->fc_w, w->fc_b, seq, yprev, state, sym + (size_t)i * R,
                       pred + (size_t)i * R, score + (size_t)i * R, beam, n_class, eos);
    DPMN_CHECK_LAUNCH();
  }
  return DPMN_OK;
}

}  // extern "C"
