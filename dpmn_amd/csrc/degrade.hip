// Synthetic LR images from HR images (dataset/dataset.py:422-489 `degradation`, :622-637 `cutblur`) for a RAGGED batch: B RGB uint8
// images of B different sizes, packed back to back; every image comes out at its own size in the same packed layout.  The semantics
// are those of utils/degrade.py degrade_u8 (the CPU reference, float64 there, fp32 here):
//   pre-blur (Gaussian 3 / 5, float) -> shot / read noise unless mean(pre-blurred) > 252 -> clip, round half to even (8 bit) ->
//   noise reduction (Gaussian 3 / 5 on the 8-bit values, rounded, or cv2's d = 7 bilateral filter) -> unsharp mask (Gaussian 3 / 5),
//   clip, truncate -> cutblur (columns on one side of cut_x are the HR image's)
// every filter with BORDER_REFLECT_101 at the IMAGE's borders; a Gaussian pass is x + sum over the taps k != centre of w[k] (x_k - x), which
// reproduces a flat region exactly (utils/degrade.py gauss_blur).
//   k_degrade<true>    per tile: the sum of the pre-blurred image over the tile's pixels -> workspace (double per tile)
//   k_degrade<false>   per tile: adds its image's partial sums in tile order (the mean > 252 test: no atomics, the same bytes on
//                      every run), then all four stages in LDS
// One block = one 32 x 32 tile of one image (host-built tile table).  The stages need 2 + 3 + 2 = 7 pixels around the tile: a stage's
// buffer holds the stage's values on the tile grown by what the later stages still need, CLIPPED TO THE IMAGE -- a tap that leaves the
// image is folded back into it, and a folded index lies in the clipped window again (|tap offset| <= the growth between two stages),
// so nothing outside the image is read or computed.  Two ping-pong buffers of at most 46 x 46 x 3 floats, pixel-interleaved: lane l of
// an element-wise pass reads dword l + const, a per-pixel pass dword 3 l + const -- both conflict-free on 32 banks.  Launch- and
// latency-bound work on a few hundred KB per batch; nothing here is tuned for throughput.
//   k_degrade_noise    the standard-normal field the fused path generates for z == NULL, written out (tests; same device function)
#include "u8_pixel.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_TILE = 32;
constexpr int DG_R_PRE = 2, DG_R_NR = 3, DG_R_SHP = 2;      // largest radius per stage: Gaussian 5, bilateral d = 7, Gaussian 5
constexpr int DG_HALO = DG_R_PRE + DG_R_NR + DG_R_SHP;
constexpr int DG_SIDE = DG_TILE + 2 * DG_HALO;              // 46
constexpr int DG_BUF = DG_SIDE * DG_SIDE * 3;
constexpr int DG_PARAMS = 16;
constexpr int DG_COLOR = 3 * 255 + 1;                        // |dR| + |dG| + |dB|
constexpr int DG_SPACE = (2 * DG_R_NR + 1) * (2 * DG_R_NR + 1);

// BORDER_REFLECT_101, folded as often as needed
__device__ __forceinline__ int fold101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// The tile grown by g pixels, clipped to the image: rows [y0, y0 + nh), columns [x0, x0 + nw).
struct Win {
  int y0, x0, nh, nw;
};
__device__ __forceinline__ Win window(int ty0, int tx0, int g, int h, int w) {
  Win r;
  r.y0 = max(ty0 - g, 0);
  r.x0 = max(tx0 - g, 0);
  r.nh = min(ty0 + DG_TILE + g, h) - r.y0;
  r.nw = min(tx0 + DG_TILE + g, w) - r.x0;
  return r;
}
// a folded image coordinate -> its index inside the window (always inside for the windows of this file; clamped all the same)
__device__ __forceinline__ int in_win(int i, int lo, int n) { return min(max(i - lo, 0), n - 1); }

// normalised Gaussian taps of size k (3 or 5) in index order
__device__ void gauss_taps(float* w, int k, float sigma) {
  float s = 0.0f;
  for (int i = 0; i < k; ++i) {
    const float d = (float)i - (float)(k - 1) * 0.5f;
    w[i] = expf(-(d * d) / (2.0f * sigma * sigma));
    s += w[i];
  }
  for (int i = 0; i < k; ++i) w[i] = w[i] / s;
}

// dst (rows of src, columns of dwin) = horizontal Gaussian of src (window swin)
__device__ void blur_hor(const float* src, const Win& swin, float* dst, const Win& dwin, const float* taps, int k, int w) {
  const int row = dwin.nw * 3, total = swin.nh * row, r = k >> 1;
  for (int e = threadIdx.x; e < total; e += DG_THREADS) {
    const int y = e / row, rem = e - y * row, x = rem / 3, c = rem - x * 3;
    const float* p = src + (size_t)y * swin.nw * 3 + c;
    const float v = p[in_win(dwin.x0 + x, swin.x0, swin.nw) * 3];
    float acc = 0.0f;
    for (int t = 0; t < k; ++t)
      if (t != r) acc += taps[t] * (p[in_win(fold101(dwin.x0 + x + t - r, w), swin.x0, swin.nw) * 3] - v);
    dst[e] = v + acc;
  }
}

// the vertical Gaussian at row y (image coordinate) of src, whose rows are those of swin and whose row length is row_len floats
__device__ __forceinline__ float blur_ver_at(const float* src, const Win& swin, int row_len, int y, int col, const float* taps, int k, int h) {
  const int r = k >> 1;
  const float v = src[(size_t)in_win(y, swin.y0, swin.nh) * row_len + col];
  float acc = 0.0f;
  for (int t = 0; t < k; ++t)
    if (t != r) acc += taps[t] * (src[(size_t)in_win(fold101(y + t - r, h), swin.y0, swin.nh) * row_len + col] - v);
  return v + acc;
}

// a standard-normal value per (seed, image, pixel, channel): splitmix64 of the counter -> two 24-bit uniforms -> Box-Muller
__device__ __forceinline__ float noise_at(unsigned long long seed, int b, int pixel, int c) {
  unsigned long long z = ((((unsigned long long)b << 26) | (unsigned long long)pixel) * 4ull + (unsigned long long)c) * DROP_PHI + seed;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u1 = ((float)(unsigned)(z >> 40) + 1.0f) * 5.9604644775390625e-8f;        // (0, 1]
  const float u2 = (float)(unsigned)((z >> 8) & 0xFFFFFFull) * 5.9604644775390625e-8f;  // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// One image as the kernels see it (include/dpmn_hip.h dpmn_degrade_ragged_u8: 4 int64 per image).  The numbers are data from the
// caller: an image or a tile that does not fit the buffers is not read and not written.
struct Item {
  long off;
  int h, w, first_tile, tiles_x, tiles;
  bool ok;
};
__device__ __forceinline__ Item load_item(const long long* __restrict__ items, int b, long packed_bytes, int n_tiles) {
  const long long* p = items + (size_t)b * 4;
  Item it;
  const long long h = p[1], w = p[2], ft = p[3];
  it.off = p[0];
  it.ok = h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && it.off >= 0 && it.off <= packed_bytes - h * w * 3 && ft >= 0 && ft < n_tiles;
  it.h = (int)h; it.w = (int)w; it.first_tile = (int)ft;
  it.tiles_x = it.ok ? (it.w + DG_TILE - 1) / DG_TILE : 0;
  it.tiles = it.ok ? it.tiles_x * ((it.h + DG_TILE - 1) / DG_TILE) : 0;
  it.ok = it.ok && it.first_tile + it.tiles <= n_tiles;
  return it;
}

// a fixed-order sum over the block: per wave the butterfly, then the four wave sums in wave order
__device__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += xshfl_v(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < DG_THREADS / 64; ++i) s += red[i];
  return s;
}

template <bool SUMS>
__global__ void __launch_bounds__(DG_THREADS)
k_degrade(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ items, const int* __restrict__ tiles,
          int n_tiles, const float* __restrict__ params, const float* __restrict__ zfield, unsigned long long seed, int B,
          unsigned char* __restrict__ out, double* __restrict__ sums) {
  __shared__ float bufA[DG_BUF], bufB[DG_BUF];
  __shared__ float taps[3][5], w_space[DG_SPACE], w_color[DG_COLOR];
  __shared__ double red[DG_THREADS / 64];
  const int tile = blockIdx.x, b = tiles[tile * 3], ty = tiles[tile * 3 + 1], tx = tiles[tile * 3 + 2];
  if (b < 0 || b >= B || ty < 0 || tx < 0) return;
  const Item it = load_item(items, b, packed_bytes, n_tiles);
  const int ty0 = ty * DG_TILE, tx0 = tx * DG_TILE;
  if (!it.ok || ty0 >= it.h || tx0 >= it.w || tile != it.first_tile + ty * it.tiles_x + tx) return;
  const int h = it.h, w = it.w;
  const float* P = params + (size_t)b * DG_PARAMS;
  const int pre_k = P[0] == 5.0f ? 5 : 3, nr_k = P[6] == 5.0f ? 5 : 3, shp_k = P[10] == 5.0f ? 5 : 3;
  const bool noise_on = P[2] != 0.0f, bilateral = P[5] != 0.0f;
  const float shot = P[3], read = P[4], gain = P[12];
  const int cut_x = (int)P[13], cut_side = (int)P[14];

  // ---- the block's weights, once
  if (threadIdx.x == 0) gauss_taps(taps[0], pre_k, P[1]);
  if (!SUMS) {
    if (threadIdx.x == 64) gauss_taps(taps[2], shp_k, P[11]);
    if (!bilateral) {
      if (threadIdx.x == 128) gauss_taps(taps[1], nr_k, P[7]);
    } else {
      const float sc = P[8], ss = P[9];
      for (int i = threadIdx.x; i < DG_COLOR; i += DG_THREADS) w_color[i] = expf(-((float)i * (float)i) / (2.0f * sc * sc));
      if (threadIdx.x < DG_SPACE) {
        const int dy = threadIdx.x / (2 * DG_R_NR + 1) - DG_R_NR, dx = threadIdx.x % (2 * DG_R_NR + 1) - DG_R_NR;
        w_space[threadIdx.x] = expf(-(float)(dx * dx + dy * dy) / (2.0f * ss * ss));
      }
    }
  }

  // ---- stage 0: the HR pixels of the tile grown by 7 -> A
  const unsigned char* src = packed + it.off;
  const Win w0 = window(ty0, tx0, DG_HALO, h, w), w1 = window(ty0, tx0, DG_HALO - DG_R_PRE, h, w);
  {
    const int row = w0.nw * 3, total = w0.nh * row;
    for (int e = threadIdx.x; e < total; e += DG_THREADS) {
      const int y = e / row, rem = e - y * row;
      bufA[e] = (float)src[((size_t)(w0.y0 + y) * w + w0.x0) * 3 + rem];
    }
  }
  __syncthreads();
  // ---- stage 1: pre-blur, A (w0) -> B (rows w0, columns w1) -> A (w1)
  blur_hor(bufA, w0, bufB, w1, taps[0], pre_k, w);
  __syncthreads();
  const int row1 = w1.nw * 3, total1 = w1.nh * row1;
  if (SUMS) {
    // the tile's own pixels only: every pixel of the image is counted by exactly one tile
    const int th = min(DG_TILE, h - ty0), tw3 = min(DG_TILE, w - tx0) * 3;
    double part = 0.0;
    for (int e = threadIdx.x; e < th * tw3; e += DG_THREADS) {
      const int y = e / tw3, rem = e - y * tw3;
      part += (double)blur_ver_at(bufB, w0, row1, ty0 + y, (tx0 - w1.x0) * 3 + rem, taps[0], pre_k, h);
    }
    const double s = block_sum(part, red);
    if (threadIdx.x == 0) sums[tile] = s;
    return;
  }
  for (int e = threadIdx.x; e < total1; e += DG_THREADS) {
    const int y = e / row1, rem = e - y * row1;
    bufA[e] = blur_ver_at(bufB, w0, row1, w1.y0 + y, rem, taps[0], pre_k, h);
  }
  // ---- the image's mean: its tiles' partial sums in tile order
  double part = 0.0;
  if (noise_on)
    for (int i = threadIdx.x; i < it.tiles; i += DG_THREADS) part += sums[it.first_tile + i];
  const bool noisy = noise_on && block_sum(part, red) / ((double)h * w * 3) <= 252.0;      // (block_sum synchronises: A is complete)
  __syncthreads();
  // ---- stage 2: noise, clip, round half to even -> A (w1), 8-bit values
  for (int e = threadIdx.x; e < total1; e += DG_THREADS) {
    float x = bufA[e];
    if (noisy) {
      const int y = e / row1, rem = e - y * row1, xx = rem / 3, c = rem - xx * 3;
      const int pixel = (w1.y0 + y) * w + w1.x0 + xx;
      const float z = zfield ? zfield[it.off + (size_t)pixel * 3 + c] : noise_at(seed, b, pixel, c);
      x = x + z * sqrtf(shot * x + read);
    }
    bufA[e] = rintf(fminf(fmaxf(x, 0.0f), 255.0f));
  }
  __syncthreads();
  // ---- stage 3: noise reduction -> nr (w2), 8-bit values
  const Win w2 = window(ty0, tx0, DG_R_SHP, h, w), w3 = window(ty0, tx0, 0, h, w);
  const int row2 = w2.nw * 3, total2 = w2.nh * row2;
  float *nr, *tmp;
  if (!bilateral) {
    blur_hor(bufA, w1, bufB, w2, taps[1], nr_k, w);
    __syncthreads();
    for (int e = threadIdx.x; e < total2; e += DG_THREADS) {
      const int y = e / row2, rem = e - y * row2;
      bufA[e] = fminf(fmaxf(rintf(blur_ver_at(bufB, w1, row2, w2.y0 + y, rem, taps[1], nr_k, h)), 0.0f), 255.0f);
    }
    nr = bufA; tmp = bufB;
  } else {
    for (int px = threadIdx.x; px < w2.nh * w2.nw; px += DG_THREADS) {
      const int y = px / w2.nw, x = px - y * w2.nw, Y = w2.y0 + y, X = w2.x0 + x;
      const float* c0 = bufA + ((size_t)(Y - w1.y0) * w1.nw + (X - w1.x0)) * 3;
      const float r0 = c0[0], g0 = c0[1], b0 = c0[2];
      float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
      for (int dy = -DG_R_NR; dy <= DG_R_NR; ++dy) {
        const int yy = in_win(fold101(Y + dy, h), w1.y0, w1.nh);
        for (int dx = -DG_R_NR; dx <= DG_R_NR; ++dx) {
          if (dx * dx + dy * dy > DG_R_NR * DG_R_NR) continue;
          const float* q = bufA + ((size_t)yy * w1.nw + in_win(fold101(X + dx, w), w1.x0, w1.nw)) * 3;
          const float r = q[0], g = q[1], bl = q[2];
          const int d = min((int)(fabsf(r - r0) + fabsf(g - g0) + fabsf(bl - b0)), DG_COLOR - 1);
          const float wt = w_space[(dy + DG_R_NR) * (2 * DG_R_NR + 1) + dx + DG_R_NR] * w_color[d];
          sr += r * wt; sg += g * wt; sb += bl * wt; sw += wt;
        }
      }
      float* o = bufB + (size_t)px * 3;
      o[0] = fminf(fmaxf(rintf(sr / sw), 0.0f), 255.0f);
      o[1] = fminf(fmaxf(rintf(sg / sw), 0.0f), 255.0f);
      o[2] = fminf(fmaxf(rintf(sb / sw), 0.0f), 255.0f);
    }
    nr = bufB; tmp = bufA;
  }
  __syncthreads();
  // ---- stage 4: unsharp mask, nr (w2) -> tmp (rows w2, columns w3) -> the tile; cutblur
  blur_hor(nr, w2, tmp, w3, taps[2], shp_k, w);
  __syncthreads();
  unsigned char* dst = out + it.off;
  const int row3 = w3.nw * 3, total3 = w3.nh * row3;
  for (int e = threadIdx.x; e < total3; e += DG_THREADS) {
    const int y = e / row3, rem = e - y * row3, xx = rem / 3, X = tx0 + xx;
    const size_t g = ((size_t)(ty0 + y) * w + tx0) * 3 + rem;
    unsigned char v;
    if ((cut_side == 1 && X >= cut_x) || (cut_side == 2 && X < cut_x)) {
      v = src[g];
    } else {
      const float lf = blur_ver_at(tmp, w2, row3, ty0 + y, rem, taps[2], shp_k, h);
      const float x = nr[((size_t)(ty0 + y - w2.y0) * w2.nw + (tx0 - w2.x0)) * 3 + rem];
      v = (unsigned char)(int)fminf(fmaxf(x + (x - lf) * gain, 0.0f), 255.0f);
    }
    dst[g] = v;
  }
}

// block (x, b): a grid-stride walk over the h x w x 3 values of image b
__global__ void __launch_bounds__(DG_THREADS)
k_degrade_noise(unsigned long long seed, const long long* __restrict__ items, long packed_bytes, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long* p = items + (size_t)b * 4;
  const long long off = p[0], h = p[1], w = p[2];
  if (h < 1 || h > RESIZE_MAX_SIDE || w < 1 || w > RESIZE_MAX_SIDE || off < 0 || off > packed_bytes - h * w * 3) return;
  const long total = (long)(h * w * 3);
  for (long i = (long)blockIdx.x * DG_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * DG_THREADS) {
    const int pixel = (int)(i / 3);
    out[off + i] = noise_at(seed, b, pixel, (int)(i - (long)pixel * 3));
  }
}

}  // namespace

extern "C" {

size_t dpmn_degrade_ragged_workspace_bytes(int n_tiles) { return n_tiles > 0 ? (size_t)n_tiles * sizeof(double) : 0; }

int dpmn_degrade_ragged_u8(const unsigned char* packed_in, long packed_bytes, const long long* items, const int* tiles, int n_tiles,
                           const float* params, const float* z_or_null, unsigned long long seed, int B, unsigned char* packed_out,
                           void* workspace, size_t workspace_bytes, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed_in && items && tiles && params && packed_out && workspace, "degrade_ragged: null pointer");
  DPMN_REQUIRE(packed_in != packed_out, "degrade_ragged: in place is not supported (tiles read their neighbours' input)");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles >= B && packed_bytes > 0, "degrade_ragged: bad sizes (1 <= B <= 65535, a tile per image at least)");
  DPMN_REQUIRE(workspace_bytes >= dpmn_degrade_ragged_workspace_bytes(n_tiles), "degrade_ragged: workspace too small");
  hipLaunchKernelGGL(k_degrade<true>, dim3((unsigned)n_tiles), dim3(DG_THREADS), 0, as_stream(stream), packed_in, packed_bytes, items, tiles,
                     n_tiles, params, z_or_null, seed, B, packed_out, (double*)workspace);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_degrade<false>, dim3((unsigned)n_tiles), dim3(DG_THREADS), 0, as_stream(stream), packed_in, packed_bytes, items, tiles,
                     n_tiles, params, z_or_null, seed, B, packed_out, (double*)workspace);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_degrade_noise_f32(unsigned long long seed, const long long* items, long packed_bytes, int B, int max_pixels, float* out,
                           dpmn_stream_t stream) {
  DPMN_REQUIRE(items && out && B > 0 && B <= 65535 && max_pixels > 0 && packed_bytes > 0, "degrade_noise: bad arguments");
  const long blocks = ((long)max_pixels * 3 + DG_THREADS - 1) / DG_THREADS;
  hipLaunchKernelGGL(k_degrade_noise, dim3((unsigned)(blocks < 256 ? blocks : 256), (unsigned)B), dim3(DG_THREADS), 0, as_stream(stream), seed,
                     items, packed_bytes, out);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
