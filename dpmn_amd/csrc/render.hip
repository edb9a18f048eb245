// HR text crops from strings (main.py --train_words): B words laid out of a glyph atlas into a RAGGED batch of RGB uint8 images, packed
// back to back in the layout of utils/resize.py pack_ragged, in ONE launch.  The semantics are those of utils/render.py render_u8 (the
// CPU reference; its docstring states every formula), integers only, so every byte is reproduced:
//   scaled advances and pen positions of the string -> undo the shear -> the glyph under the pixel -> integer bilinear sample of its
//   alpha cell (Q16, round half up) -> background (flat or a linear gradient, + grain from the counter hash of degrade.hip) -> blend
// One block = one 8 x 128 tile of one image (host-built tile table, as degrade.hip), a lane = 4 neighbouring pixels of a row.  The block
// stages the string's cells, advances and pen positions in LDS once and finds the glyph under the tile's leftmost text column once; a
// pixel walks on from there (the text column grows with x), never from column 0.  A lane stores its 12 bytes as three dwords where the
// row's first byte is dword-aligned in memory, byte by byte otherwise and for the last w % 4 pixels of a row.
// Launch- and latency-bound work on a few hundred KB per batch.
#include "u8_pixel.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE_H = 8, RD_TILE_W = 128;      // RD_THREADS lanes x 4 pixels
constexpr int RD_MAX_LEN = 25;
constexpr int RD_N_GLYPH = 37;
constexpr int RD_PARAMS = 24;
// columns of a params row (utils/render.py)
constexpr int P_FONT = 0, P_CASE = 1, P_GH = 2, P_SPACING = 3, P_LEFT = 4, P_RIGHT = 5, P_TOP = 6, P_SHEAR = 8, P_FG = 9, P_BG = 12, P_STYLE = 15,
              P_BG2 = 16, P_SEED = 19;

// atlas coordinate of the scaled index i along one axis: pixel centres, Q16, clamped to [0, limit]
__device__ __forceinline__ void axis_sample(int i, long long sc, int limit, int& i0, int& i1, long long& frac) {
  long long q = (((2ll * i + 1) * sc) >> 1) - 32768;
  if (q < 0) q = 0;
  i0 = min((int)(q >> 16), limit);
  i1 = min(i0 + 1, limit);
  frac = q & 0xFFFF;
}

__device__ __forceinline__ int grain_at(unsigned long long seed, unsigned long long pixel) {
  unsigned long long z = (pixel * 4ull) * DROP_PHI + seed;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)((z >> 40) % 9ull) - 4;
}

__global__ void __launch_bounds__(RD_THREADS)
k_render_words(const int* __restrict__ classes, const int* __restrict__ lengths, const long long* __restrict__ params,
               const unsigned char* __restrict__ atlas, const int* __restrict__ advance, const int* __restrict__ atlas_h,
               const long long* __restrict__ items, const int* __restrict__ tiles, int n_tiles, unsigned char* __restrict__ out,
               long out_bytes, int B, int n_fonts, int GH, int GW) {
  __shared__ int s_pen[RD_MAX_LEN + 1], s_adv[RD_MAX_LEN], s_cellw[RD_MAX_LEN];
  __shared__ long s_cell[RD_MAX_LEN];
  __shared__ int s_first;
  const int tile = blockIdx.x;
  if (tile >= n_tiles) return;
  const int b = tiles[tile * 3], ty = tiles[tile * 3 + 1], tx = tiles[tile * 3 + 2];
  if (b < 0 || b >= B || ty < 0 || tx < 0) return;
  // ---- the image: numbers from the caller, so an image or a tile that does not fit the buffer is not written
  const long long* it = items + (size_t)b * 4;
  const long long off = it[0], h64 = it[1], w64 = it[2];
  if (h64 < 1 || h64 > RESIZE_MAX_SIDE || w64 < 1 || w64 > RESIZE_MAX_SIDE || off < 0 || off > out_bytes - h64 * w64 * 3) return;
  const int h = (int)h64, w = (int)w64;
  const int ty0 = ty * RD_TILE_H, tx0 = tx * RD_TILE_W;
  if (ty0 >= h || tx0 >= w) return;
  const long long* P = params + (size_t)b * RD_PARAMS;
  const int f = min(max((int)P[P_FONT], 0), n_fonts - 1), cs = (int)P[P_CASE], gh = max((int)P[P_GH], 1), sp = (int)P[P_SPACING];
  const int left = (int)P[P_LEFT], top = (int)P[P_TOP], s = (int)P[P_SHEAR], style = (int)P[P_STYLE];
  const int A = min(max(atlas_h[f], 1), GH);
  const int n = min(max(lengths[b], 1), RD_MAX_LEN);
  const int room = (int)(((long long)abs(s) * gh + 65535) >> 16);
  const int x0 = left + (s < 0 ? room : 0), base = top + gh - 1;

  // ---- the string, once per block: cells, scaled advances, pen positions, the glyph under the tile's leftmost text column
  if (threadIdx.x < n) {
    const int k = threadIdx.x;
    const int c = min(max(classes[b * RD_MAX_LEN + k], 0), RD_N_GLYPH - 1);
    const int plane = (cs == 1 || (cs == 2 && k == 0)) ? 1 : 0;
    const int cell = (f * 2 + plane) * RD_N_GLYPH + c;
    const int adv = min(max(advance[cell], 1), GW);
    s_cell[k] = (long)cell * GH * GW;
    s_cellw[k] = adv;
    s_adv[k] = max(1, (int)(((long long)adv * gh + A / 2) / A));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int pen = 0;
    for (int k = 0; k < n; ++k) { s_pen[k] = pen; pen += max(s_adv[k] + sp, 0); }
    s_pen[n] = pen;
    // the smallest text column of the tile: its first pixel column under the largest shift of its rows (the shift is monotonic in y)
    const int y_last = min(ty0 + RD_TILE_H, h) - 1;
    const int shift = max((s * (base - ty0)) >> 16, (s * (base - y_last)) >> 16);
    const int u_min = tx0 - shift - x0;
    int k = 0;
    while (k + 1 < n && u_min >= s_pen[k + 1]) ++k;
    s_first = k;
  }
  __syncthreads();

  const int y = ty0 + (int)(threadIdx.x >> 5), x = tx0 + (int)(threadIdx.x & 31) * 4;
  if (y >= h || x >= w) return;
  const int npx = min(4, w - x);
  const int tw = max(s_pen[n] - sp, 1);
  const int v = y - top, u_row = x - ((s * (base - y)) >> 16) - x0;
  const long long sc = ((long long)A << 16) / gh;
  const unsigned long long seed = (unsigned long long)P[P_SEED];
  int fg[3], bg[3], bg2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    fg[c] = min(max((int)P[P_FG + c], 0), 255);
    bg[c] = min(max((int)P[P_BG + c], 0), 255);
    bg2[c] = min(max((int)P[P_BG2 + c], 0), 255);
  }
  int y_0 = 0, y_1 = 0;
  long long fy = 0;
  const bool row_in = v >= 0 && v < gh;
  if (row_in) axis_sample(v, sc, A - 1, y_0, y_1, fy);

  unsigned int word[3] = {0u, 0u, 0u};      // the lane's 12 bytes, little endian
  int k = s_first;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= npx) break;
    const int u = u_row + i;
    int alpha = 0;
    if (row_in && u >= 0 && u < tw) {
      while (k + 1 < n && u >= s_pen[k + 1]) ++k;
      const int ug = u - s_pen[k];
      if (ug >= 0 && ug < s_adv[k]) {
        int x_0, x_1;
        long long fx;
        axis_sample(ug, sc, s_cellw[k] - 1, x_0, x_1, fx);
        const unsigned char* cell = atlas + s_cell[k];
        const long long a00 = cell[y_0 * GW + x_0], a01 = cell[y_0 * GW + x_1], a10 = cell[y_1 * GW + x_0], a11 = cell[y_1 * GW + x_1];
        const unsigned long long t = (unsigned long long)(a00 * (65536 - fx) + a01 * fx), bt = (unsigned long long)(a10 * (65536 - fx) + a11 * fx);
        alpha = (int)((t * (unsigned long long)(65536 - fy) + bt * (unsigned long long)fy + (1ull << 31)) >> 32);
      }
    }
    const int g = grain_at(seed, (unsigned long long)y * (unsigned long long)w + (unsigned long long)(x + i));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int back = bg[c];
      if (style == 1) {
        const int m = max(w - 1, 1);
        back = (bg[c] * (m - (x + i)) + bg2[c] * (x + i) + m / 2) / m;
      } else if (style == 2) {
        const int m = max(h - 1, 1);
        back = (bg[c] * (m - y) + bg2[c] * y + m / 2) / m;
      }
      back = min(max(back + g, 0), 255);
      const unsigned int val = (unsigned int)((fg[c] * alpha + back * (255 - alpha) + 127) / 255);
      const int byte = i * 3 + c;
      word[byte >> 2] |= val << ((byte & 3) * 8);
    }
  }
  unsigned char* dst = out + off + ((size_t)y * w + x) * 3;
  if (npx == 4 && ((size_t)dst & 3) == 0) {
    unsigned int* d4 = reinterpret_cast<unsigned int*>(dst);
    d4[0] = word[0]; d4[1] = word[1]; d4[2] = word[2];
  } else {
#pragma unroll
    for (int byte = 0; byte < 12; ++byte)
      if (byte < npx * 3) dst[byte] = (unsigned char)(word[byte >> 2] >> ((byte & 3) * 8));
  }
}

}  // namespace

// ---- Outline, drop shadow and photo background (main.py --train_words_fx): the semantics of utils/render.py render_fx_u8, beside the
// plain kernel above, which stays as it is.  Same 8 x 128 tiles, same tile table, same packed layout, ONE launch.  A block first
// evaluates the plain alpha of its tile plus a 3-pixel halo (14 x 134 bytes, 0 outside the canvas) into LDS -- the atlas is sampled once
// per pixel; after the barrier the outline's dilation (the largest alpha over a disk of radius <= 3), the shadow's one shifted tap and
// the fill read LDS.  The photo background is four reads per channel from the pool (the crop sampled at the pixel's centre, the integer
// bilinear blend of the alpha), pulled toward the drawn background before the grain.  Integers only: the same bytes in every compute mode.
namespace {

constexpr int FX_COLS = 20, FX_HALO = 3;
constexpr int FX_ROWS = RD_TILE_H + 2 * FX_HALO, FX_USED = RD_TILE_W + 2 * FX_HALO, FX_STRIDE = FX_USED + 2;      // 14 rows of 134 (136) bytes
// columns of an fx row (utils/render.py)
constexpr int F_FLAGS = 0, F_R = 1, F_OUTLINE = 2, F_DX = 5, F_DY = 6, F_Q = 7, F_SHADOW = 8, F_PHOTO = 11, F_X0 = 12, F_Y0 = 13, F_CW = 14,
              F_CH = 15, F_M = 16;

__device__ __forceinline__ int over(int colour, int a, int c) { return (colour * a + c * (255 - a) + 127) / 255; }

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return (int)min(max(v, (long long)lo), (long long)hi); }

// the integer bilinear blend of one alpha cell, round half up (utils/render.py: alpha)
__device__ __forceinline__ int cell_alpha(const unsigned char* cell, int GW, int x_0, int x_1, int y_0, int y_1, long long fx_, long long fy_) {
  const long long a00 = cell[y_0 * GW + x_0], a01 = cell[y_0 * GW + x_1], a10 = cell[y_1 * GW + x_0], a11 = cell[y_1 * GW + x_1];
  const unsigned long long t = (unsigned long long)(a00 * (65536 - fx_) + a01 * fx_), bt = (unsigned long long)(a10 * (65536 - fx_) + a11 * fx_);
  return (int)((t * (unsigned long long)(65536 - fy_) + bt * (unsigned long long)fy_ + (1ull << 31)) >> 32);
}

// ---- Projective distortion, rotation and a curved baseline (main.py --train_words_warp): the semantics of utils/render.py
// render_warp_u8 (the comment above N_WARP states every formula and the bound that keeps every intermediate below 2^62).
constexpr int WP_COLS = 16;
// columns of a warp row (utils/render.py)
constexpr int W_FLAGS = 0, W_AMP = 1, W_ROOM = 2, W_COEF = 3, W_H = 12, W_W = 13;
constexpr long long WP_COEF_MAX = 1ll << 30, WP_AMP_MAX = (1ll << 23) - 1;

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// floor(a / b) for b > 0: C++ truncates toward 0, the restatement floors
__device__ __forceinline__ long long floordiv(long long a, long long b) {
  const long long q = a / b;
  return (a - q * b < 0) ? q - 1 : q;
}

// atlas coordinate of the Q16 position pos along one axis (axis_sample at a fractional index)
__device__ __forceinline__ void warp_sample(long long pos, long long sc, int limit, int& i0, int& i1, long long& frac) {
  long long q = ((pos * sc) >> 16) - 32768;
  if (q < 0) q = 0;
  i0 = (int)min(q >> 16, (long long)limit);
  i1 = min(i0 + 1, limit);
  frac = q & 0xFFFF;
}

struct WarpRow {
  long long c[9], amp, off;      // off: room << 16 for a word that arches upward
  int w0;                        // width of the flat canvas
};

// The alpha of output pixel (x, y) of a warped sample: two int64 floor divisions to the Q16 position on the bent flat canvas, the
// parabola, the shear at the fractional row, a binary search of the pens in LDS for the LAST k with pen_k <= u (the walk from the
// tile's leftmost column does not hold under a warp), the fractional atlas sample.
__device__ __forceinline__ int warp_alpha(const WarpRow& wr, int x, int y, int top, int gh, int s, int x0, int tw, int n, const int* s_pen,
                                          const int* s_adv, const int* s_cellw, const long* s_cell, const unsigned char* atlas, long long sc,
                                          int A, int GW) {
  const long long X = 2ll * x + 1, Y = 2ll * y + 1;
  const long long den = wr.c[6] * X + wr.c[7] * Y + 2 * wr.c[8];
  if (den <= 0) return 0;
  const long long px = floordiv((wr.c[0] * X + wr.c[1] * Y + 2 * wr.c[2]) * 65536, den);
  if (px < 0 || px >= ((long long)wr.w0 << 16)) return 0;
  const long long py = floordiv((wr.c[3] * X + wr.c[4] * Y + 2 * wr.c[5]) * 65536, den);
  long long p = 0;
  if (wr.amp != 0) {
    const long long xq = px >> 12, Wq = (long long)wr.w0 << 4;
    p = floordiv(wr.amp * 4 * xq * (Wq - xq), Wq * Wq);
  }
  const long long vq = py - wr.off - p - ((long long)top << 16);
  if (vq < 0 || vq >= ((long long)gh << 16)) return 0;
  const long long uq = px - (((long long)s * ((((long long)gh - 1) << 16) + 32768 - vq)) >> 16) - ((long long)x0 << 16);
  if (uq < 0 || uq >= ((long long)tw << 16)) return 0;
  const int u = (int)(uq >> 16);
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_pen[mid] <= u) lo = mid; else hi = mid - 1;
  }
  const long long ugq = uq - ((long long)s_pen[lo] << 16);
  if (ugq < 0 || ugq >= ((long long)s_adv[lo] << 16)) return 0;
  int x_0, x_1, y_0, y_1;
  long long fx_, fy_;
  warp_sample(ugq, sc, s_cellw[lo] - 1, x_0, x_1, fx_);
  warp_sample(vq, sc, A - 1, y_0, y_1, fy_);
  return cell_alpha(atlas + s_cell[lo], GW, x_0, x_1, y_0, y_1, fx_, fy_);
}

// One tile of k_render_words_fx (WARP = false) and of k_render_words_warp (WARP = true: a sample whose warp flags are not 0 takes
// warp_alpha for its alpha plane; everything behind the plane is the same code).
template <bool WARP>
__device__ __forceinline__ void
render_fx_tile(const int* __restrict__ classes, const int* __restrict__ lengths, const long long* __restrict__ params,
               const long long* __restrict__ fx, const long long* __restrict__ warp, const unsigned char* __restrict__ atlas,
               const int* __restrict__ advance, const int* __restrict__ atlas_h, const long long* __restrict__ items,
               const int* __restrict__ tiles, int n_tiles, const unsigned char* __restrict__ pool, long pool_bytes,
               const long long* __restrict__ photos, int n_photos, unsigned char* __restrict__ out, long out_bytes, int B, int n_fonts,
               int GH, int GW) {
  __shared__ int s_pen[RD_MAX_LEN + 1], s_adv[RD_MAX_LEN], s_cellw[RD_MAX_LEN];
  __shared__ long s_cell[RD_MAX_LEN];
  __shared__ int s_first;
  __shared__ unsigned char s_alpha[FX_ROWS * FX_STRIDE];
  const int tile = blockIdx.x;
  if (tile >= n_tiles) return;
  const int b = tiles[tile * 3], ty = tiles[tile * 3 + 1], tx = tiles[tile * 3 + 2];
  if (b < 0 || b >= B || ty < 0 || tx < 0) return;
  // ---- the image: numbers from the caller, so an image or a tile that does not fit the buffer is not written (block-uniform returns)
  const long long* it = items + (size_t)b * 4;
  const long long off = it[0], h64 = it[1], w64 = it[2];
  if (h64 < 1 || h64 > RESIZE_MAX_SIDE || w64 < 1 || w64 > RESIZE_MAX_SIDE || off < 0 || off > out_bytes - h64 * w64 * 3) return;
  const int h = (int)h64, w = (int)w64;
  const int ty0 = ty * RD_TILE_H, tx0 = tx * RD_TILE_W;
  if (ty0 >= h || tx0 >= w) return;
  const long long* P = params + (size_t)b * RD_PARAMS;
  const int f = min(max((int)P[P_FONT], 0), n_fonts - 1), cs = (int)P[P_CASE], gh = max((int)P[P_GH], 1), sp = (int)P[P_SPACING];
  const int left = (int)P[P_LEFT], top = (int)P[P_TOP], s = (int)P[P_SHEAR], style = (int)P[P_STYLE];
  const int A = min(max(atlas_h[f], 1), GH);
  const int n = min(max(lengths[b], 1), RD_MAX_LEN);
  const int room = (int)(((long long)abs(s) * gh + 65535) >> 16);
  const int x0 = left + (s < 0 ? room : 0), base = top + gh - 1;

  // ---- the string, once per block, as the plain kernel stages it; the glyph under the leftmost text column of the tile AND its halo
  if (threadIdx.x < n) {
    const int k = threadIdx.x;
    const int c = min(max(classes[b * RD_MAX_LEN + k], 0), RD_N_GLYPH - 1);
    const int plane = (cs == 1 || (cs == 2 && k == 0)) ? 1 : 0;
    const int cell = (f * 2 + plane) * RD_N_GLYPH + c;
    const int adv = min(max(advance[cell], 1), GW);
    s_cell[k] = (long)cell * GH * GW;
    s_cellw[k] = adv;
    s_adv[k] = max(1, (int)(((long long)adv * gh + A / 2) / A));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int pen = 0;
    for (int k = 0; k < n; ++k) { s_pen[k] = pen; pen += max(s_adv[k] + sp, 0); }
    s_pen[n] = pen;
    const int y_a = ty0 - FX_HALO, y_b = min(ty0 + RD_TILE_H, h) - 1 + FX_HALO;
    const int shift = max((s * (base - y_a)) >> 16, (s * (base - y_b)) >> 16);
    const int u_min = tx0 - FX_HALO - shift - x0;
    int k = 0;
    while (k + 1 < n && u_min >= s_pen[k + 1]) ++k;
    s_first = k;
  }
  __syncthreads();

  // ---- the alpha of the tile and its halo -> LDS, every thread (no thread has left the block yet)
  const int tw = max(s_pen[n] - sp, 1);
  const long long sc = ((long long)A << 16) / gh;
  // the warp row, block-uniform; what is read of it is clamped to its domain (the coefficients to the bound of the 2^62 argument)
  bool warped = false;
  WarpRow wr = {};
  if (WARP) {
    const long long* Wr = warp + (size_t)b * WP_COLS;
    warped = Wr[W_FLAGS] != 0;
    if (warped) {
#pragma unroll
      for (int c = 0; c < 9; ++c) wr.c[c] = clampll(Wr[W_COEF + c], -WP_COEF_MAX, WP_COEF_MAX);
      wr.amp = (Wr[W_FLAGS] & 4) ? clampll(Wr[W_AMP], -WP_AMP_MAX, WP_AMP_MAX) : 0;
      wr.off = wr.amp < 0 ? clampll(Wr[W_ROOM], 0, RESIZE_MAX_SIDE) << 16 : 0;
      wr.w0 = clampi((long long)left + tw + room + clampll(P[P_RIGHT], 0, RESIZE_MAX_SIDE), 1, RESIZE_MAX_SIDE);
    }
  }
  for (int idx = threadIdx.x; idx < FX_ROWS * FX_USED; idx += RD_THREADS) {
    const int ly = idx / FX_USED, lx = idx - ly * FX_USED;
    const int y = ty0 - FX_HALO + ly, x = tx0 - FX_HALO + lx;
    int alpha = 0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      if (WARP && warped) {
        alpha = warp_alpha(wr, x, y, top, gh, s, x0, tw, n, s_pen, s_adv, s_cellw, s_cell, atlas, sc, A, GW);
      } else {
        const int v = y - top, u = x - ((s * (base - y)) >> 16) - x0;
        if (v >= 0 && v < gh && u >= 0 && u < tw) {
          int k = s_first;
          while (k + 1 < n && u >= s_pen[k + 1]) ++k;
          const int ug = u - s_pen[k];
          if (ug >= 0 && ug < s_adv[k]) {
            int x_0, x_1, y_0, y_1;
            long long fx_, fy_;
            axis_sample(ug, sc, s_cellw[k] - 1, x_0, x_1, fx_);
            axis_sample(v, sc, A - 1, y_0, y_1, fy_);
            alpha = cell_alpha(atlas + s_cell[k], GW, x_0, x_1, y_0, y_1, fx_, fy_);
          }
        }
      }
    }
    s_alpha[ly * FX_STRIDE + lx] = (unsigned char)alpha;
  }
  __syncthreads();

  const int y = ty0 + (int)(threadIdx.x >> 5), x = tx0 + (int)(threadIdx.x & 31) * 4;
  if (y >= h || x >= w) return;
  const int npx = min(4, w - x);
  const unsigned long long seed = (unsigned long long)P[P_SEED];
  const long long* F = fx + (size_t)b * FX_COLS;
  const int flags = (int)F[F_FLAGS];
  // what is read of a row is clamped to its domain: the taps stay inside the halo, the crop inside its photo, the photo inside the pool
  const int r = (flags & 1) ? clampi(F[F_R], 1, FX_HALO) : 0;
  const int dx = clampi(F[F_DX], -FX_HALO, FX_HALO), dy = clampi(F[F_DY], -FX_HALO, FX_HALO), q = (flags & 2) ? clampi(F[F_Q], 0, 255) : 0;
  int fg[3], bg[3], bg2[3], oc[3], sh[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    fg[c] = min(max((int)P[P_FG + c], 0), 255);
    bg[c] = min(max((int)P[P_BG + c], 0), 255);
    bg2[c] = min(max((int)P[P_BG2 + c], 0), 255);
    oc[c] = clampi(F[F_OUTLINE + c], 0, 255);
    sh[c] = clampi(F[F_SHADOW + c], 0, 255);
  }
  bool tex = (flags & 4) != 0 && n_photos > 0 && pool != nullptr;
  const unsigned char* photo = pool;
  int pw = 1, cw = 1, ch = 1, cx = 0, m = 0, cy_0 = 0, cy_1 = 0;
  long long fcy = 0, scx = 0;
  if (tex) {
    const long long* ph_ = photos + (size_t)clampi(F[F_PHOTO], 0, n_photos - 1) * 3;
    const long long poff = ph_[0], ph64 = ph_[1], pw64 = ph_[2];
    tex = ph64 >= 1 && ph64 <= RESIZE_MAX_SIDE && pw64 >= 1 && pw64 <= RESIZE_MAX_SIDE && poff >= 0 && poff <= pool_bytes - ph64 * pw64 * 3;
    if (tex) {
      const int ph = (int)ph64;
      pw = (int)pw64;
      cw = clampi(F[F_CW], 1, pw);
      ch = clampi(F[F_CH], 1, ph);
      cx = clampi(F[F_X0], 0, pw - cw);
      const int cy = clampi(F[F_Y0], 0, ph - ch);
      m = clampi(F[F_M], 0, 256);
      photo = pool + poff + ((size_t)cy * pw + cx) * 3;
      scx = ((long long)cw << 16) / w;
      axis_sample(y, ((long long)ch << 16) / h, ch - 1, cy_0, cy_1, fcy);
    }
  }

  unsigned int word[3] = {0u, 0u, 0u};      // the lane's 12 bytes, little endian
  const unsigned char* a_row = s_alpha + (y - ty0 + FX_HALO) * FX_STRIDE + (x - tx0 + FX_HALO);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= npx) break;
    const unsigned char* a_c = a_row + i;
    const int alpha = a_c[0];
    const int a_s = ((int)a_c[-dy * FX_STRIDE - dx] * q + 127) / 255;
    int a_o = 0;
    for (int j = -r; j <= r && r > 0; ++j)
      for (int e = -r; e <= r; ++e)
        if (e * e + j * j <= r * r) a_o = max(a_o, (int)a_c[j * FX_STRIDE + e]);
    int cx_0 = 0, cx_1 = 0;
    long long fcx = 0;
    if (tex) axis_sample(x + i, scx, cw - 1, cx_0, cx_1, fcx);
    const int g = grain_at(seed, (unsigned long long)y * (unsigned long long)w + (unsigned long long)(x + i));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int back = bg[c];
      if (style == 1) {
        const int mm = max(w - 1, 1);
        back = (bg[c] * (mm - (x + i)) + bg2[c] * (x + i) + mm / 2) / mm;
      } else if (style == 2) {
        const int mm = max(h - 1, 1);
        back = (bg[c] * (mm - y) + bg2[c] * y + mm / 2) / mm;
      }
      if (tex) {
        const unsigned char* r0 = photo + (size_t)cy_0 * pw * 3 + c;
        const unsigned char* r1 = photo + (size_t)cy_1 * pw * 3 + c;
        const long long p00 = r0[cx_0 * 3], p01 = r0[cx_1 * 3], p10 = r1[cx_0 * 3], p11 = r1[cx_1 * 3];
        const unsigned long long t = (unsigned long long)(p00 * (65536 - fcx) + p01 * fcx), bt = (unsigned long long)(p10 * (65536 - fcx) + p11 * fcx);
        const int texel = (int)((t * (unsigned long long)(65536 - fcy) + bt * (unsigned long long)fcy + (1ull << 31)) >> 32);
        back = (texel * m + back * (256 - m) + 128) >> 8;
      }
      int v = min(max(back + g, 0), 255);
      v = over(sh[c], a_s, v);
      v = over(oc[c], a_o, v);
      const unsigned int val = (unsigned int)over(fg[c], alpha, v);
      const int byte = i * 3 + c;
      word[byte >> 2] |= val << ((byte & 3) * 8);
    }
  }
  unsigned char* dst = out + off + ((size_t)y * w + x) * 3;
  if (npx == 4 && ((size_t)dst & 3) == 0) {
    unsigned int* d4 = reinterpret_cast<unsigned int*>(dst);
    d4[0] = word[0]; d4[1] = word[1]; d4[2] = word[2];
  } else {
#pragma unroll
    for (int byte = 0; byte < 12; ++byte)
      if (byte < npx * 3) dst[byte] = (unsigned char)(word[byte >> 2] >> ((byte & 3) * 8));
  }
}

__global__ void __launch_bounds__(RD_THREADS)
k_render_words_fx(const int* __restrict__ classes, const int* __restrict__ lengths, const long long* __restrict__ params,
                  const long long* __restrict__ fx, const unsigned char* __restrict__ atlas, const int* __restrict__ advance,
                  const int* __restrict__ atlas_h, const long long* __restrict__ items, const int* __restrict__ tiles, int n_tiles,
                  const unsigned char* __restrict__ pool, long pool_bytes, const long long* __restrict__ photos, int n_photos,
                  unsigned char* __restrict__ out, long out_bytes, int B, int n_fonts, int GH, int GW) {
  render_fx_tile<false>(classes, lengths, params, fx, nullptr, atlas, advance, atlas_h, items, tiles, n_tiles, pool, pool_bytes, photos,
                        n_photos, out, out_bytes, B, n_fonts, GH, GW);
}

// items: the canvas of a warped sample is its warp row's H x W (utils/render.py render_warp_meta)
__global__ void __launch_bounds__(RD_THREADS)
k_render_words_warp(const int* __restrict__ classes, const int* __restrict__ lengths, const long long* __restrict__ params,
                    const long long* __restrict__ fx, const long long* __restrict__ warp, const unsigned char* __restrict__ atlas,
                    const int* __restrict__ advance, const int* __restrict__ atlas_h, const long long* __restrict__ items,
                    const int* __restrict__ tiles, int n_tiles, const unsigned char* __restrict__ pool, long pool_bytes,
                    const long long* __restrict__ photos, int n_photos, unsigned char* __restrict__ out, long out_bytes, int B,
                    int n_fonts, int GH, int GW) {
  render_fx_tile<true>(classes, lengths, params, fx, warp, atlas, advance, atlas_h, items, tiles, n_tiles, pool, pool_bytes, photos,
                       n_photos, out, out_bytes, B, n_fonts, GH, GW);
}

int check_fx_batch(int n_tiles, const unsigned char* pool_u8, long pool_bytes, const long long* photos, int n_photos, long out_bytes, int B,
                   int n_fonts, int GH, int GW, const int* host_classes, const int* host_lengths, const long long* host_params,
                   const long long* host_fx, const long long* host_meta, const long long* host_photos);

}  // namespace

extern "C" {

int dpmn_render_words_u8(const int* classes, const int* lengths, const long long* params, const unsigned char* atlas_u8, const int* advance,
                         const int* atlas_h, const long long* meta, const int* tiles, int n_tiles, unsigned char* out_packed, long out_bytes,
                         int B, int n_fonts, int GH, int GW, const int* host_classes, const int* host_lengths, const long long* host_params,
                         const long long* host_meta, dpmn_stream_t stream) {
  DPMN_REQUIRE(classes && lengths && params && atlas_u8 && advance && atlas_h && meta && tiles && out_packed, "render_words: null pointer");
  DPMN_REQUIRE(host_classes && host_lengths && host_params && host_meta, "render_words: the host copies of classes, lengths, params and meta are required (they are checked here)");
  DPMN_REQUIRE(B > 0 && B <= 65535, "render_words: bad batch size (1 <= B <= 65535)");
  DPMN_REQUIRE(n_fonts > 0 && GH > 0 && GH <= 256 && GW > 0 && GW <= 1024, "render_words: bad atlas (fonts >= 1, cell 1 .. 256 x 1 .. 1024)");
  DPMN_REQUIRE(n_tiles >= B && out_bytes > 0, "render_words: bad sizes (a tile per image at least)");
  long n_expected = 0;
  for (int b = 0; b < B; ++b) {
    DPMN_REQUIRE(host_lengths[b] >= 1 && host_lengths[b] <= RD_MAX_LEN, "render_words: a word's length is outside 1 .. 25");
    for (int k = 0; k < host_lengths[b]; ++k)
      DPMN_REQUIRE(host_classes[b * RD_MAX_LEN + k] >= 0 && host_classes[b * RD_MAX_LEN + k] < RD_N_GLYPH, "render_words: a class outside the atlas (0 .. 36)");
    const long long* P = host_params + (size_t)b * RD_PARAMS;
    DPMN_REQUIRE(P[P_FONT] >= 0 && P[P_FONT] < n_fonts, "render_words: a font index out of range");
    DPMN_REQUIRE(P[P_GH] >= 1 && P[P_GH] <= 256 && P[P_SHEAR] >= -65536 && P[P_SHEAR] <= 65536 && P[P_SPACING] >= -1 && P[P_SPACING] <= 64 &&
                 P[P_LEFT] >= 0 && P[P_LEFT] <= RESIZE_MAX_SIDE && P[P_TOP] >= 0 && P[P_TOP] <= RESIZE_MAX_SIDE,
                 "render_words: a params row is outside its domain");
    const long long off = host_meta[b * 4], h = host_meta[b * 4 + 1], w = host_meta[b * 4 + 2];
    DPMN_REQUIRE(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE, "render_words: an image side outside 1 .. 8192");
    DPMN_REQUIRE(off >= 0 && off <= out_bytes - h * w * 3, "render_words: an image lies outside the output buffer");
    n_expected += ((h + RD_TILE_H - 1) / RD_TILE_H) * ((w + RD_TILE_W - 1) / RD_TILE_W);
  }
  DPMN_REQUIRE(n_expected == n_tiles, "render_words: the tile table does not cover the images (8 x 128 tiles)");
  hipLaunchKernelGGL(k_render_words, dim3((unsigned)n_tiles), dim3(RD_THREADS), 0, as_stream(stream), classes, lengths, params, atlas_u8,
                     advance, atlas_h, meta, tiles, n_tiles, out_packed, out_bytes, B, n_fonts, GH, GW);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_render_words_fx_u8(const int* classes, const int* lengths, const long long* params, const long long* fx, const unsigned char* atlas_u8,
                            const int* advance, const int* atlas_h, const long long* meta, const int* tiles, int n_tiles,
                            const unsigned char* pool_u8, long pool_bytes, const long long* photos, int n_photos, unsigned char* out_packed,
                            long out_bytes, int B, int n_fonts, int GH, int GW, const int* host_classes, const int* host_lengths,
                            const long long* host_params, const long long* host_fx, const long long* host_meta, const long long* host_photos,
                            dpmn_stream_t stream) {
  DPMN_REQUIRE(classes && lengths && params && fx && atlas_u8 && advance && atlas_h && meta && tiles && out_packed, "render_words_fx: null pointer");
  const int rc = check_fx_batch(n_tiles, pool_u8, pool_bytes, photos, n_photos, out_bytes, B, n_fonts, GH, GW, host_classes, host_lengths,
                                host_params, host_fx, host_meta, host_photos);
  if (rc != DPMN_OK) return rc;
  hipLaunchKernelGGL(k_render_words_fx, dim3((unsigned)n_tiles), dim3(RD_THREADS), 0, as_stream(stream), classes, lengths, params, fx, atlas_u8,
                     advance, atlas_h, meta, tiles, n_tiles, pool_u8, pool_bytes, photos, n_photos, out_packed, out_bytes, B, n_fonts, GH, GW);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"

namespace {

// the host checks of dpmn_render_words_fx_u8, which dpmn_render_words_warp_u8 makes too
int check_fx_batch(int n_tiles, const unsigned char* pool_u8, long pool_bytes, const long long* photos, int n_photos, long out_bytes, int B,
                   int n_fonts, int GH, int GW, const int* host_classes, const int* host_lengths, const long long* host_params,
                   const long long* host_fx, const long long* host_meta, const long long* host_photos) {
  DPMN_REQUIRE(host_classes && host_lengths && host_params && host_fx && host_meta, "render_words_fx: the host copies of classes, lengths, params, fx and meta are required (they are checked here)");
  DPMN_REQUIRE(B > 0 && B <= 65535, "render_words_fx: bad batch size (1 <= B <= 65535)");
  DPMN_REQUIRE(n_fonts > 0 && GH > 0 && GH <= 256 && GW > 0 && GW <= 1024, "render_words_fx: bad atlas (fonts >= 1, cell 1 .. 256 x 1 .. 1024)");
  DPMN_REQUIRE(n_tiles >= B && out_bytes > 0, "render_words_fx: bad sizes (a tile per image at least)");
  DPMN_REQUIRE(n_photos >= 0 && pool_bytes >= 0 && (n_photos == 0 || (pool_u8 && photos && host_photos)), "render_words_fx: a pool of photos needs its bytes and both copies of its table");
  for (int k = 0; k < n_photos; ++k) {
    const long long off = host_photos[k * 3], h = host_photos[k * 3 + 1], w = host_photos[k * 3 + 2];
    DPMN_REQUIRE(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && off >= 0 && off <= pool_bytes - h * w * 3,
                 "render_words_fx: a photo lies outside the pool or has a side outside 1 .. 8192");
  }
  long n_expected = 0;
  for (int b = 0; b < B; ++b) {
    DPMN_REQUIRE(host_lengths[b] >= 1 && host_lengths[b] <= RD_MAX_LEN, "render_words_fx: a word's length is outside 1 .. 25");
    for (int k = 0; k < host_lengths[b]; ++k)
      DPMN_REQUIRE(host_classes[b * RD_MAX_LEN + k] >= 0 && host_classes[b * RD_MAX_LEN + k] < RD_N_GLYPH, "render_words_fx: a class outside the atlas (0 .. 36)");
    const long long* P = host_params + (size_t)b * RD_PARAMS;
    DPMN_REQUIRE(P[P_FONT] >= 0 && P[P_FONT] < n_fonts, "render_words_fx: a font index out of range");
    DPMN_REQUIRE(P[P_GH] >= 1 && P[P_GH] <= 256 && P[P_SHEAR] >= -65536 && P[P_SHEAR] <= 65536 && P[P_SPACING] >= -1 && P[P_SPACING] <= 64 &&
                 P[P_LEFT] >= 0 && P[P_LEFT] <= RESIZE_MAX_SIDE && P[P_TOP] >= 0 && P[P_TOP] <= RESIZE_MAX_SIDE,
                 "render_words_fx: a params row is outside its domain");
    const long long off = host_meta[b * 4], h = host_meta[b * 4 + 1], w = host_meta[b * 4 + 2];
    DPMN_REQUIRE(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE, "render_words_fx: an image side outside 1 .. 8192");
    DPMN_REQUIRE(off >= 0 && off <= out_bytes - h * w * 3, "render_words_fx: an image lies outside the output buffer");
    n_expected += ((h + RD_TILE_H - 1) / RD_TILE_H) * ((w + RD_TILE_W - 1) / RD_TILE_W);
    // the fx row: the columns of the kinds whose flag bit is set (utils/render.py check_render_fx)
    const long long* F = host_fx + (size_t)b * FX_COLS;
    DPMN_REQUIRE(F[F_FLAGS] >= 0 && F[F_FLAGS] <= 7 && F[F_M + 1] == 0 && F[F_M + 2] == 0 && F[F_M + 3] == 0,
                 "render_words_fx: flags outside 0 .. 7, or a spare column that is not 0");
    if (F[F_FLAGS] & 1) {
      DPMN_REQUIRE(F[F_R] >= 1 && F[F_R] <= FX_HALO, "render_words_fx: an outline radius outside 1 .. 3");
      for (int c = 0; c < 3; ++c) DPMN_REQUIRE(F[F_OUTLINE + c] >= 0 && F[F_OUTLINE + c] <= 255, "render_words_fx: an outline colour outside 0 .. 255");
    }
    if (F[F_FLAGS] & 2) {
      DPMN_REQUIRE(F[F_DX] >= -FX_HALO && F[F_DX] <= FX_HALO && F[F_DY] >= -FX_HALO && F[F_DY] <= FX_HALO && (F[F_DX] != 0 || F[F_DY] != 0),
                   "render_words_fx: a shadow offset outside -3 .. 3, or (0, 0)");
      DPMN_REQUIRE(F[F_Q] >= 96 && F[F_Q] <= 255, "render_words_fx: a shadow opacity outside 96 .. 255");
      for (int c = 0; c < 3; ++c) DPMN_REQUIRE(F[F_SHADOW + c] >= 0 && F[F_SHADOW + c] <= 255, "render_words_fx: a shadow colour outside 0 .. 255");
    }
    if (F[F_FLAGS] & 4) {
      DPMN_REQUIRE(F[F_PHOTO] >= 0 && F[F_PHOTO] < n_photos, "render_words_fx: a photo index outside the pool");
      const long long ph = host_photos[F[F_PHOTO] * 3 + 1], pw = host_photos[F[F_PHOTO] * 3 + 2];
      DPMN_REQUIRE(F[F_X0] >= 0 && F[F_Y0] >= 0 && F[F_CW] >= 1 && F[F_CH] >= 1 && F[F_CW] <= pw - F[F_X0] && F[F_CH] <= ph - F[F_Y0],
                   "render_words_fx: a crop leaves its photo");
      DPMN_REQUIRE(F[F_M] >= 64 && F[F_M] <= 224, "render_words_fx: a blend weight outside 64 .. 224");
    }
  }
  DPMN_REQUIRE(n_expected == n_tiles, "render_words_fx: the tile table does not cover the images (8 x 128 tiles)");
  return DPMN_OK;
}

}  // namespace

extern "C" {

int dpmn_render_words_warp_u8(const int* classes, const int* lengths, const long long* params, const long long* fx, const long long* warp,
                              const unsigned char* atlas_u8, const int* advance, const int* atlas_h, const long long* meta, const int* tiles,
                              int n_tiles, const unsigned char* pool_u8, long pool_bytes, const long long* photos, int n_photos,
                              unsigned char* out_packed, long out_bytes, int B, int n_fonts, int GH, int GW, const int* host_classes,
                              const int* host_lengths, const long long* host_params, const long long* host_fx, const long long* host_warp,
                              const long long* host_meta, const long long* host_photos, dpmn_stream_t stream) {
  DPMN_REQUIRE(classes && lengths && params && fx && warp && atlas_u8 && advance && atlas_h && meta && tiles && out_packed, "render_words_warp: null pointer");
  DPMN_REQUIRE(host_warp, "render_words_warp: the host copy of the warp rows is required (it is checked here)");
  const int rc = check_fx_batch(n_tiles, pool_u8, pool_bytes, photos, n_photos, out_bytes, B, n_fonts, GH, GW, host_classes, host_lengths,
                                host_params, host_fx, host_meta, host_photos);
  if (rc != DPMN_OK) return rc;
  // the warp rows whose flags are not 0 (utils/render.py check_render_warp)
  for (int b = 0; b < B; ++b) {
    const long long* Wr = host_warp + (size_t)b * WP_COLS;
    DPMN_REQUIRE(Wr[W_FLAGS] >= 0 && Wr[W_FLAGS] <= 7, "render_words_warp: flags outside 0 .. 7");
    if (Wr[W_FLAGS] == 0) continue;
    DPMN_REQUIRE(Wr[W_W + 1] == 0 && Wr[W_W + 2] == 0, "render_words_warp: a spare column that is not 0");
    for (int c = 0; c < 9; ++c)
      DPMN_REQUIRE(Wr[W_COEF + c] >= -WP_COEF_MAX && Wr[W_COEF + c] <= WP_COEF_MAX, "render_words_warp: a coefficient of the map passes 2^30 (an intermediate could pass 2^62)");
    const long long H = Wr[W_H], W = Wr[W_W];
    DPMN_REQUIRE(H == host_meta[b * 4 + 1] && W == host_meta[b * 4 + 2], "render_words_warp: the canvas of a warped sample is not its row's H x W");
    for (int k = 0; k < 4; ++k)
      DPMN_REQUIRE(Wr[W_COEF + 6] * ((k & 1) ? W : 0) + Wr[W_COEF + 7] * ((k & 2) ? H : 0) + Wr[W_COEF + 8] > 0, "render_words_warp: den <= 0 at a corner of the output canvas");
    const long long amp = Wr[W_AMP] < 0 ? -Wr[W_AMP] : Wr[W_AMP], gh = host_params[(size_t)b * RD_PARAMS + P_GH];
    DPMN_REQUIRE((Wr[W_FLAGS] & 4) ? amp <= WP_AMP_MAX && amp * 10 <= 4 * 65536 * gh : amp == 0, "render_words_warp: amp outside its range (|amp| <= 0.4 gh in Q16 with the curve bit, 0 without it)");
    DPMN_REQUIRE(Wr[W_ROOM] == ((amp + 65535) >> 16), "render_words_warp: room is not ceil(|amp|)");
  }
  hipLaunchKernelGGL(k_render_words_warp, dim3((unsigned)n_tiles), dim3(RD_THREADS), 0, as_stream(stream), classes, lengths, params, fx, warp,
                     atlas_u8, advance, atlas_h, meta, tiles, n_tiles, pool_u8, pool_bytes, photos, n_photos, out_packed, out_bytes, B, n_fonts,
                     GH, GW);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
