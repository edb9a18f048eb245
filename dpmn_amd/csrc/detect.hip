// The text regions of a photo without a box file (utils/detect.py fixes the semantics; main.py --demo_detect): a RAGGED batch of RGB
// uint8 photos (resize.hip's packed layout) -> per photo the gradient map, its histogram, the smoothed binary map, the component
// labels and a table of the components' bounding boxes and pixel counts.  Integers only: independent of the compute mode, and every
// map byte for byte the numpy restatement.  Every kernel walks the same table of 64 x 16 tiles of the WORKING maps (hm x wm =
// H // r x W // r, r = ceil(max(H, W) / 1024)), one block of 4 waves per tile: a wave owns 4 rows of the tile, a lane one column, so a
// wave's ballot over "is foreground" IS the 64-pixel word of its row.
//   k_detect_grad     box-reduce + luma + 3 x 3 max - min in one launch: the tile's Y with a 1-pixel halo is staged in LDS once and the
//                     9 taps are read from there; the histogram is counted in LDS and added to the photo's 256 counters.
//   k_detect_hsmooth  g >= T and the run-length smoothing of the rows: per row of the tile the 3 words x0 - 64 .. x0 + 128 in LDS; a
//                     pixel finds its nearest foreground on either side with clz / ffs on two shifted words (gap <= 64).
//   k_detect_cell_otsu, k_detect_hsmooth_local  (the locally adaptive threshold, off by default) Otsu's threshold per cell of the working
//                     map, found on the device, and k_detect_hsmooth against the threshold map interpolated between the cell centres.
//   k_detect_vsmooth  the same down the columns: the words of the rows y0 - vgap .. y0 + 16 + vgap in LDS, a lane walks its bit up and
//                     down at most vgap words.  Also the initial label: the least index of the pixel's run inside its word.
//   k_detect_union    label equivalence: neighbours are united by atomicMin on roots.  One pass over the edges.
//   k_detect_roots    a pixel that is its own label is a root: it takes a row of the photo's table (atomicAdd on the photo's counter).
//   k_detect_stats    every pixel finds its root, stores it (the flattened label) and adds itself to the root's row with integer
//                     atomicMin / atomicMax / atomicAdd, which commute; a word whose pixels share one root sends one update.
//   k_detect_moments  (oriented regions) every pixel adds x, y, x^2, x y, y^2 to its component's int64 row with 64-bit atomicAdd; a word
//                     with one root reduces x and x^2 over the wave and its leading lane sends one update per sum.
//   k_detect_extents  (oriented regions) atomicMax of the projections of the pixel centres along and across the component's direction,
//                     which the host chose from the moments; in a word with one root its first and last pixel give the extremes.
//   k_detect_profile  (bowed lines) per component and vertical bin of its box the least and greatest y, the pixel count and the sum of y,
//                     with 32-bit atomicMax / atomicAdd; in a word with one root one update per bin segment of the word.
// Termination: a label only ever decreases (atomicMin) and L[i] <= i holds from the start, so find() follows a strictly decreasing
// chain of non-negative indices and stops (it also stops at any value that is not below its index, whatever the buffer holds); an
// iteration of unite() that does not return replaces one of its two roots by a strictly smaller one and find() never increases one, so
// the sum of the two decreases and the loop ends.  No launch is repeated "until nothing changes": one union pass is complete, because a
// link that an atomicMin overwrites is re-established by the thread that sees the overwritten value.
#include "u8_pixel.h"

namespace {

constexpr int DT_W = 64, DT_H = 16, DT_THREADS = 256, DT_WAVES = 4, DT_WAVE_ROWS = DT_H / DT_WAVES;
constexpr int DETECT_ITEM_WORDS = 8, DETECT_MAP_SIDE = 1024, DETECT_MAX_GAP = 64, DETECT_ROW = 5;
typedef unsigned long long u64;

// One photo as the kernels see it (include/dpmn_hip.h: 8 int64 per photo).  The numbers are data from the caller: an item that is not
// consistent with the buffers is not touched.  packed_bytes < 0: the photo itself is not read by this launch.
__host__ __device__ inline bool detect_item_ok(const long long* p, long packed_bytes, long map_px) {
  const long long in_off = p[0], H = p[1], W = p[2], map_off = p[3], hm = p[4], wm = p[5], r = p[6];
  if (!(H >= 1 && H <= RESIZE_MAX_SIDE && W >= 1 && W <= RESIZE_MAX_SIDE)) return false;
  if (r != ((H > W ? H : W) + DETECT_MAP_SIDE - 1) / DETECT_MAP_SIDE || hm != H / r || wm != W / r) return false;
  if (packed_bytes >= 0 && !(in_off >= 0 && in_off <= packed_bytes - H * W * 3)) return false;
  return map_off >= 0 && map_off <= map_px - hm * wm;
}

struct DetTile {
  int b, x0, y0, hm, wm, r, W;
  long long in_off, map_off;
};

// The block's tile; false (for the whole block) when the tile names no photo, a bad item or a place outside its map.
__device__ inline bool detect_tile(const long long* __restrict__ items, int B, const int* __restrict__ tiles, long packed_bytes, long map_px,
                                   DetTile& t) {
  const int* q = tiles + (size_t)blockIdx.x * 3;
  const int b = q[0], tr = q[1], tc = q[2];
  if (b < 0 || b >= B) return false;
  const long long* p = items + (size_t)b * DETECT_ITEM_WORDS;
  if (!detect_item_ok(p, packed_bytes, map_px)) return false;
  t.b = b; t.in_off = p[0]; t.W = (int)p[2]; t.map_off = p[3]; t.hm = (int)p[4]; t.wm = (int)p[5]; t.r = (int)p[6];
  if (t.hm < 1 || t.wm < 1 || tr < 0 || tc < 0 || tr > (t.hm - 1) / DT_H || tc > (t.wm - 1) / DT_W) return false;
  t.x0 = tc * DT_W; t.y0 = tr * DT_H;
  return true;
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_grad(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ items, int B,
              const int* __restrict__ tiles, unsigned char* __restrict__ g, long map_px, unsigned* __restrict__ hist) {
  __shared__ unsigned char sY[DT_H + 2][DT_W + 4];
  __shared__ unsigned sHist[256];
  DetTile t;
  if (!detect_tile(items, B, tiles, packed_bytes, map_px, t)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  sHist[tid] = 0;
  const unsigned char* src = packed + t.in_off;
  const int r = t.r, rr = r * r, half = rr / 2;
  for (int i = tid; i < (DT_H + 2) * (DT_W + 2); i += DT_THREADS) {
    const int ly = i / (DT_W + 2), lx = i - ly * (DT_W + 2);
    // (edges replicated: the halo outside the map repeats the border pixel, so every read stays inside the photo)
    const int my = min(max(t.y0 + ly - 1, 0), t.hm - 1), mx = min(max(t.x0 + lx - 1, 0), t.wm - 1);
    const unsigned char* p = src + ((size_t)my * r * t.W + (size_t)mx * r) * 3;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int dy = 0; dy < r; ++dy) {
      const unsigned char* q = p + (size_t)dy * t.W * 3;
      for (int dx = 0; dx < r; ++dx, q += 3) {
        s0 += q[0];
        s1 += q[1];
        s2 += q[2];
      }
    }
    const int R = (s0 + half) / rr, G = (s1 + half) / rr, Bc = (s2 + half) / rr;
    sY[ly][lx] = (unsigned char)((77 * R + 150 * G + 29 * Bc + 128) >> 8);
  }
  __syncthreads();
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int ly = wave * DT_WAVE_ROWS + k, y = t.y0 + ly;
    if (x < t.wm && y < t.hm) {
      int mx = 0, mn = 255;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int v = sY[ly + dy][lane + dx];
          mx = max(mx, v);
          mn = min(mn, v);
        }
      g[t.map_off + (size_t)y * t.wm + x] = (unsigned char)(mx - mn);
      atomicAdd(&sHist[mx - mn], 1u);
    }
  }
  __syncthreads();
  if (sHist[tid]) atomicAdd(&hist[(size_t)t.b * 256 + tid], sHist[tid]);
}

// The run-length smoothing of the rows of a tile from the words of its ballots (sW[row] = the words at x0 - 64, x0, x0 + 64), shared by
// the two kernels that threshold.
__device__ inline void detect_smooth_rows(const u64 (*sW)[3], const DetTile& t, int lane, int wave, int gap, unsigned char* __restrict__ out) {
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int ly = wave * DT_WAVE_ROWS + k, y = t.y0 + ly;
    if (x >= t.wm || y >= t.hm) continue;
    const u64 w0 = sW[ly][0], w1 = sW[ly][1], w2 = sW[ly][2];
    bool f = (w1 >> lane) & 1;
    if (!f) {
      // Lm: bit 63 is the pixel at x - 1, bit 63 - i the one at x - 1 - i; Rm: bit 0 is the pixel at x + 1, bit i the one at x + 1 + i
      const u64 Lm = (lane ? w1 << (64 - lane) : 0ull) | (w0 >> lane);
      const u64 Rm = ((w1 >> lane) >> 1) | (w2 << (63 - lane));
      if (Lm && Rm) f = __clzll((long long)Lm) + __ffsll((long long)Rm) <= gap;      // dl + dr - 1, dl = clz + 1, dr = ffs
    }
    out[t.map_off + (size_t)y * t.wm + x] = f ? 1 : 0;
  }
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_hsmooth(const unsigned char* __restrict__ g, long map_px, const long long* __restrict__ items, int B, const int* __restrict__ tiles,
                 const int* __restrict__ thresholds, int gap, unsigned char* __restrict__ out) {
  __shared__ u64 sW[DT_H][3];
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = thresholds[t.b];
  const unsigned char* src = g + t.map_off;
  for (int i = wave; i < DT_H * 3; i += DT_WAVES) {
    const int ly = i / 3, k = i - ly * 3, y = t.y0 + ly, x = t.x0 + (k - 1) * DT_W + lane;
    const bool f = y < t.hm && x >= 0 && x < t.wm && (int)src[(size_t)y * t.wm + x] >= T;
    const u64 m = __ballot(f);
    if (lane == 0) sW[ly][k] = m;
  }
  __syncthreads();
  detect_smooth_rows(sW, t, lane, wave, gap, out);
}

// ---- the locally adaptive threshold (utils/detect.py, local = C): one Otsu threshold per cell of the working map, bilinear between the
// cell centres.  Per axis of `size` pixels n = ceil(size / C) cells with the edges e_i = i * size / n; a photo's ny * nx thresholds lie
// at word 7 of its item in one int32 table of n_cells entries, photo after photo in the order of the items.

__host__ __device__ inline int detect_cells(int size, int C) { return (size + C - 1) / C; }

// Word 7 of an item against the table: false unless the photo's cells lie inside it.
__host__ __device__ inline bool detect_cells_ok(const long long* p, int C, long n_cells) {
  const long long at = p[7], n = (long long)detect_cells((int)p[4], C) * detect_cells((int)p[5], C);
  return at >= 0 && at <= n_cells - n;
}

// One pixel of one axis: the two cells k and k1 around it and their weights, w0 + w1 = D <= size <= 1024 (D = e_{k+2} - e_k).
struct DetAxis {
  int k, k1, w0, w1;
};

__device__ inline DetAxis detect_axis(int x, int size, int C) {
  const int n = detect_cells(size, C);
  DetAxis a = {0, 0, 1, 0};
  if (n < 2 || x < 0 || x >= size) return a;
  const int j = ((x + 1) * n - 1) / size;                                  // the pixel's own cell: e_j <= x < e_{j+1}
  const int p = 2 * x + 1, cj = j * size / n + (j + 1) * size / n;       // doubled: the pixel's centre and the cell's
  const int k = min(max(p >= cj ? j : j - 1, 0), n - 2);                  // the greatest k with c_k <= p, capped
  const int ck = k * size / n + (k + 1) * size / n, ck1 = (k + 1) * size / n + (k + 2) * size / n;
  const int q = min(max(p, ck), ck1);                                      // (outside the outermost centres: their own value)
  a.k = k; a.k1 = k + 1; a.w0 = ck1 - q; a.w1 = q - ck;
  return a;
}

// T(y, x) = (2 sum of the four w_y w_x t + Dy Dx) / (2 Dy Dx), rounded half up.  t <= 255 and D <= 1024 per axis, so the numerator is
// at most 511 * 2^20 < 2^31: 32-bit arithmetic is exact.
__device__ inline int detect_local_T(const int* __restrict__ cell, int nx, const DetAxis& ay, const DetAxis& ax) {
  const int* r0 = cell + ay.k * nx;
  const int* r1 = cell + ay.k1 * nx;
  const int s = ay.w0 * (ax.w0 * r0[ax.k] + ax.w1 * r0[ax.k1]) + ay.w1 * (ax.w0 * r1[ax.k] + ax.w1 * r1[ax.k1]);
  const int dd = (ay.w0 + ay.w1) * (ax.w0 + ax.w1);
  return (int)((unsigned)(2 * s + dd) / (unsigned)(2 * dd));
}

// k_detect_hsmooth with every pixel compared against its own T(y, x), the halo words at x0 - 64 and x0 + 64 included: the weights of the
// tile's 192 columns and 16 rows are worked out once per block into LDS, the four cell thresholds of a pixel come from the photo's
// table.  tmap (may be null; for tests): T of the tile's own pixels, int32 (map_px).
__global__ void __launch_bounds__(DT_THREADS)
k_detect_hsmooth_local(const unsigned char* __restrict__ g, long map_px, const long long* __restrict__ items, int B,
                       const int* __restrict__ tiles, const int* __restrict__ table, long n_cells, int C, int gap,
                       unsigned char* __restrict__ out, int* __restrict__ tmap) {
  __shared__ u64 sW[DT_H][3];
  __shared__ DetAxis sX[3 * DT_W], sY[DT_H];
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  const long long* item = items + (size_t)t.b * DETECT_ITEM_WORDS;
  if (!detect_cells_ok(item, C, n_cells)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* cell = table + item[7];
  const int nx = detect_cells(t.wm, C);
  if (tid < 3 * DT_W) sX[tid] = detect_axis(t.x0 - DT_W + tid, t.wm, C);
  else if (tid < 3 * DT_W + DT_H) sY[tid - 3 * DT_W] = detect_axis(t.y0 + tid - 3 * DT_W, t.hm, C);
  __syncthreads();
  const unsigned char* src = g + t.map_off;
  for (int i = wave; i < DT_H * 3; i += DT_WAVES) {
    const int ly = i / 3, k = i - ly * 3, y = t.y0 + ly, x = t.x0 + (k - 1) * DT_W + lane;
    bool f = false;
    if (y < t.hm && x >= 0 && x < t.wm) {
      const int T = detect_local_T(cell, nx, sY[ly], sX[k * DT_W + lane]);
      f = (int)src[(size_t)y * t.wm + x] >= T;
      if (tmap && k == 1) tmap[t.map_off + (size_t)y * t.wm + x] = T;
    }
    const u64 m = __ballot(f);
    if (lane == 0) sW[ly][k] = m;
  }
  __syncthreads();
  detect_smooth_rows(sW, t, lane, wave, gap, out);
}

// One block per (photo, cell): the histogram of g over the cell in LDS (a copy per wave, so that a flat cell does not serialise the whole
// block on one counter), then wave 0 finds Otsu's t -> table[cell] = max(t + 1, floor).  The block finds its photo from word 7 of the
// items, which the entry point checked to be the running sum of the photos' cell counts (16 halvings: B <= 65535).
// The comparison is utils.detect.otsu's, exact: candidate (a, b) = ((S0 N - S N0)^2, N0 N1) beats (num, den) when a den > num b.  With
// N <= 2^20 pixels of at most 255: S < 2^28, |S0 N - S N0| < 2^48, a < 2^96, b < 2^40, and a product a * b' < 2^136 does not fit 128
// bits.  It is held in three limbs: a = ah 2^64 + al (ah < 2^32), a b' = (ah b' + (al b' >> 64)) 2^64 + (al b' mod 2^64), the upper
// part below 2^73, so unsigned __int128 holds each part and two products compare part by part.  No floating point.
typedef unsigned __int128 u128;

struct DetProduct {
  u128 hi;
  u64 lo;
};

__device__ inline DetProduct detect_mul(u128 a, u64 b) {
  const u128 low = (u128)(u64)a * b;
  DetProduct p = {(u128)(u64)(a >> 64) * b + (low >> 64), (u64)low};
  return p;
}

// a den > num b
__device__ inline bool detect_ratio_gt(u128 a, u64 b, u128 num, u64 den) {
  const DetProduct l = detect_mul(a, den), r = detect_mul(num, b);
  return l.hi > r.hi || (l.hi == r.hi && l.lo > r.lo);
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_cell_otsu(const unsigned char* __restrict__ g, long map_px, const long long* __restrict__ items, int B, int C, int floor_,
                   int* __restrict__ table, long n_cells) {
  __shared__ unsigned sH[DT_WAVES][256];
  const long idx = (long)blockIdx.x;
  if (idx >= n_cells) return;
  int b = 0;
  for (int step = 1 << 15; step; step >>= 1)      // the greatest photo whose first cell is not past this one
    if (b + step < B && items[(size_t)(b + step) * DETECT_ITEM_WORDS + 7] <= idx) b += step;
  const long long* item = items + (size_t)b * DETECT_ITEM_WORDS;
  if (!detect_item_ok(item, -1, map_px) || !detect_cells_ok(item, C, n_cells)) return;
  const int hm = (int)item[4], wm = (int)item[5], ny = detect_cells(hm, C), nx = detect_cells(wm, C);
  const long long rel = idx - item[7];
  if (rel < 0 || rel >= (long long)ny * nx) return;
  const int cy = (int)(rel / nx), cx = (int)(rel - (long long)cy * nx);
  const int y0 = cy * hm / ny, y1 = (cy + 1) * hm / ny, x0 = cx * wm / nx, x1 = (cx + 1) * wm / nx;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int w = 0; w < DT_WAVES; ++w) sH[w][tid] = 0;
  __syncthreads();
  const unsigned char* src = g + item[3];
  for (int y = y0 + wave; y < y1; y += DT_WAVES)      // a wave per row, a lane per column: every read stays inside the cell
    for (int x = x0 + lane; x < x1; x += 64) atomicAdd(&sH[wave][src[(size_t)y * wm + x]], 1u);
  __syncthreads();
  if (wave) return;
  // lane l owns the bins 4 l .. 4 l + 3; N0 and S0 before its first bin come from a prefix sum over the wave
  unsigned h[4], n = 0, s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = sH[0][4 * lane + j] + sH[1][4 * lane + j] + sH[2][4 * lane + j] + sH[3][4 * lane + j];
    n += h[j];
    s += (unsigned)(4 * lane + j) * h[j];
  }
  unsigned pn = n, ps = s;      // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned un = __shfl_up(pn, d), us = __shfl_up(ps, d);
    if (lane >= d) {
      pn += un;
      ps += us;
    }
  }
  const long long N = __shfl(pn, 63), S = __shfl(ps, 63);
  long long N0 = pn - n, S0 = ps - s;
  int best = 0;
  u128 num = 0;
  u64 den = 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    N0 += h[j];
    S0 += (long long)(4 * lane + j) * h[j];
    const long long N1 = N - N0;
    if (N0 == 0 || N1 == 0) continue;
    const long long d = S0 * N - S * N0;
    const u64 ad = (u64)(d < 0 ? -d : d), bb = (u64)N0 * (u64)N1;
    const u128 a = (u128)ad * ad;
    if (detect_ratio_gt(a, bb, num, den)) {
      best = 4 * lane + j;
      num = a;
      den = bb;
    }
  }
  // the greatest ratio of the wave, the earliest t on a tie (a lane without a candidate holds 0 / 1 at t = 0, which is otsu's start)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int ot = __shfl_xor(best, d);
    const u64 nl = __shfl_xor((u64)num, d), nh = __shfl_xor((u64)(num >> 64), d), od = __shfl_xor(den, d);
    const u128 on = ((u128)nh << 64) | nl;
    const bool gt = detect_ratio_gt(on, od, num, den), lt = detect_ratio_gt(num, den, on, od);
    if (gt || (!lt && ot < best)) {
      best = ot;
      num = on;
      den = od;
    }
  }
  if (lane == 0) table[idx] = max(best + 1, floor_);
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_vsmooth(const unsigned char* __restrict__ in, long map_px, const long long* __restrict__ items, int B, const int* __restrict__ tiles,
                 int vgap, unsigned char* __restrict__ smooth, int* __restrict__ labels) {
  __shared__ u64 sR[DT_H + 2 * DETECT_MAX_GAP];
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned char* src = in + t.map_off;
  const int x = t.x0 + lane;
  for (int i = wave; i < DT_H + 2 * vgap; i += DT_WAVES) {
    const int y = t.y0 - vgap + i;
    const bool f = y >= 0 && y < t.hm && x < t.wm && src[(size_t)y * t.wm + x] != 0;
    const u64 m = __ballot(f);
    if (lane == 0) sR[i] = m;
  }
  __syncthreads();
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int ly = wave * DT_WAVE_ROWS + k, y = t.y0 + ly, c = ly + vgap;
    const bool inside = x < t.wm && y < t.hm;
    bool f = (sR[c] >> lane) & 1;
    if (!f) {
      int du = 0, dd = 0;
      for (int i = 1; i <= vgap; ++i) {
        if (!du && ((sR[c - i] >> lane) & 1)) du = i;
        if (!dd && ((sR[c + i] >> lane) & 1)) dd = i;
      }
      f = du && dd && du + dd - 1 <= vgap;
    }
    f = f && inside;
    const u64 word = __ballot(f);
    if (!inside) continue;
    const size_t idx = t.map_off + (size_t)y * t.wm + x;
    smooth[idx] = f ? 1 : 0;
    int lab = -1;
    if (f) {      // the least index of the pixel's run inside this word: below it, and in the pixel's component
      const u64 z = ~word & ((1ull << lane) - 1);
      lab = y * t.wm + t.x0 + (z ? 64 - __clzll((long long)z) : 0);
    }
    labels[idx] = lab;
  }
}

// The root of i: the chain L[i] > L[L[i]] > ... ends at the first index that is its own label.  A value that is not below its index
// (never written by these kernels) ends it too, so the walk is bounded by i whatever the buffer holds.
__device__ inline int detect_find(int* L, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= i || p < 0) return i;
    i = p;
  }
}

__device__ inline void detect_unite(int* L, int a, int b) {
  for (;;) {
    a = detect_find(L, a);
    b = detect_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&L[a], b);      // a was a root when find read it: link it below b
    if (old == a) return;
    a = old;      // another thread linked a first (old < a): what it linked a to joins b in the next turn
  }
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_union(const unsigned char* __restrict__ smooth, int* __restrict__ labels, long map_px, const long long* __restrict__ items, int B,
               const int* __restrict__ tiles) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned char* S = smooth + t.map_off;
  int* L = labels + t.map_off;
  const int x = t.x0 + lane, wm = t.wm;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;
    if (x >= wm || y >= t.hm) continue;
    const int i = y * wm + x;
    if (!S[i]) continue;
    if (lane == 0 && x > 0 && S[i - 1]) detect_unite(L, i, i - 1);      // (inside a word the run already shares its label)
    if (y > 0) {
      // the pixel above joins its own neighbours along its row: the two diagonals matter only where it is background
      if (S[i - wm]) detect_unite(L, i, i - wm);
      else {
        if (x > 0 && S[i - wm - 1]) detect_unite(L, i, i - wm - 1);
        if (x + 1 < wm && S[i - wm + 1]) detect_unite(L, i, i - wm + 1);
      }
    }
  }
}

// slices: int64 (B, 2) per photo [first row of its table, rows it may use]
__device__ inline bool detect_slice(const long long* __restrict__ slices, int b, long table_rows, long long& first, long long& cap) {
  first = slices[(size_t)b * 2];
  cap = slices[(size_t)b * 2 + 1];
  return first >= 0 && cap >= 0 && first <= table_rows - cap;
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_roots(const int* __restrict__ labels, long map_px, const long long* __restrict__ items, int B, const int* __restrict__ tiles,
               const long long* __restrict__ slices, int* __restrict__ counts, int* __restrict__ slots, int* __restrict__ table, long table_rows) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  long long first, cap;
  if (!detect_slice(slices, t.b, table_rows, first, cap)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;
    if (x >= t.wm || y >= t.hm) continue;
    const int i = y * t.wm + x;
    if (labels[t.map_off + i] != i) continue;
    const int slot = atomicAdd(&counts[t.b], 1);      // (the counter goes on past cap: the caller learns how many rows it needs)
    if (slot < cap) {
      int* row = table + (size_t)(first + slot) * DETECT_ROW;
      row[0] = x; row[1] = y; row[2] = x; row[3] = y; row[4] = 0;
    }
    slots[t.map_off + i] = slot < cap ? slot : -1;
  }
}

__global__ void __launch_bounds__(DT_THREADS)
k_detect_stats(const unsigned char* __restrict__ smooth, int* __restrict__ labels, long map_px, const long long* __restrict__ items, int B,
               const int* __restrict__ tiles, const long long* __restrict__ slices, const int* __restrict__ slots, int* __restrict__ table,
               long table_rows) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  long long first, cap;
  if (!detect_slice(slices, t.b, table_rows, first, cap)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* L = labels + t.map_off;
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;      // (uniform over the wave: every lane reaches the ballots)
    const bool f = x < t.wm && y < t.hm && smooth[t.map_off + (size_t)y * t.wm + x] != 0;
    int root = -1, slot = -1;
    if (f) {
      root = detect_find(L, y * t.wm + x);
      L[y * t.wm + x] = root;
      slot = slots[t.map_off + root];
      if (slot >= cap) slot = -1;
    }
    const u64 word = __ballot(f);
    if (!word) continue;
    const int lead = __ffsll((long long)word) - 1, root0 = __shfl(root, lead);
    const bool one = __ballot(f && root != root0) == 0;
    if (!f || slot < 0) continue;
    int* row = table + (size_t)(first + slot) * DETECT_ROW;
    if (one) {      // the word's pixels share a root: its leading lane sends their extent and count
      if (lane != lead) continue;
      atomicMin(&row[0], t.x0 + lead);
      atomicMax(&row[2], t.x0 + 63 - __clzll((long long)word));
      atomicMin(&row[1], y);
      atomicMax(&row[3], y);
      atomicAdd(&row[4], __popcll(word));
    } else {
      atomicMin(&row[0], x);
      atomicMax(&row[2], x);
      atomicMin(&row[1], y);
      atomicMax(&row[3], y);
      atomicAdd(&row[4], 1);
    }
  }
}

// The oriented regions (utils/detect.py, stages a and c) read what k_detect_stats left: labels[pixel] = root, slots[root] = table row.
// The word of a wave's row, its root test and the row of the table, as k_detect_stats finds them; false for the whole wave when the
// word is empty.  slot < 0: this lane adds nothing.
__device__ inline bool detect_word(const unsigned char* __restrict__ smooth, const int* __restrict__ labels, const int* __restrict__ slots,
                                   const DetTile& t, int x, int y, long long cap, bool& f, u64& word, bool& one, int& slot) {
  f = x < t.wm && y < t.hm && smooth[t.map_off + (size_t)y * t.wm + x] != 0;
  int root = -1;
  slot = -1;
  if (f) {
    root = labels[t.map_off + (size_t)y * t.wm + x];
    if (root >= 0 && root < t.hm * t.wm) slot = slots[t.map_off + root];      // (a label that is no index of the map names no row)
    if (slot >= cap) slot = -1;
  }
  word = __ballot(f);
  if (!word) return false;
  const int root0 = __shfl(root, __ffsll((long long)word) - 1);
  one = __ballot(f && root != root0) == 0;
  return true;
}

// table: u64 (table_rows, 5) [sum x, sum y, sum x^2, sum x y, sum y^2] per component (the area is in the table of k_detect_stats),
// zeroed by the entry point.  Every sum of a word is below 2^31; the table's are below 2^60.
__global__ void __launch_bounds__(DT_THREADS)
k_detect_moments(const unsigned char* __restrict__ smooth, const int* __restrict__ labels, long map_px, const long long* __restrict__ items,
                 int B, const int* __restrict__ tiles, const long long* __restrict__ slices, const int* __restrict__ slots,
                 u64* __restrict__ table, long table_rows) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  long long first, cap;
  if (!detect_slice(slices, t.b, table_rows, first, cap)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;      // (uniform over the wave: every lane reaches the ballots and the shuffles)
    bool f, one;
    u64 word;
    int slot;
    if (!detect_word(smooth, labels, slots, t, x, y, cap, f, word, one, slot)) continue;
    if (one) {      // one root: sum x and sum x^2 over the set bits by a wave reduction, the rest follows from y and the popcount
      int sx = f ? x : 0, sxx = f ? x * x : 0;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        sx += __shfl_xor(sx, d);
        sxx += __shfl_xor(sxx, d);
      }
      if (lane != __ffsll((long long)word) - 1 || slot < 0) continue;
      u64* row = table + (size_t)(first + slot) * 5;
      const u64 n = (u64)__popcll(word);
      atomicAdd(&row[0], (u64)sx);
      atomicAdd(&row[1], (u64)y * n);
      atomicAdd(&row[2], (u64)sxx);
      atomicAdd(&row[3], (u64)y * (u64)sx);
      atomicAdd(&row[4], (u64)y * (u64)y * n);
    } else if (f && slot >= 0) {
      u64* row = table + (size_t)(first + slot) * 5;
      atomicAdd(&row[0], (u64)x);
      atomicAdd(&row[1], (u64)y);
      atomicAdd(&row[2], (u64)(x * x));
      atomicAdd(&row[3], (u64)(x * y));
      atomicAdd(&row[4], (u64)(y * y));
    }
  }
}

// dirs: int32 (table_rows, 2) per component (c, s) of its direction, (0, 0): the component is passed over.  table: int32
// (table_rows, 4) [max -U2, max U2, max -V2, max V2], U2 = c (2x + 1) + s (2y + 1), V2 = -s (2x + 1) + c (2y + 1) (below 2^27 in
// magnitude), every byte set to 0x80 by the entry point: a value below every projection, so that four atomicMax do it.
__global__ void __launch_bounds__(DT_THREADS)
k_detect_extents(const unsigned char* __restrict__ smooth, const int* __restrict__ labels, long map_px, const long long* __restrict__ items,
                 int B, const int* __restrict__ tiles, const long long* __restrict__ slices, const int* __restrict__ slots,
                 const int* __restrict__ dirs, int* __restrict__ table, long table_rows) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  long long first, cap;
  if (!detect_slice(slices, t.b, table_rows, first, cap)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;
    bool f, one;
    u64 word;
    int slot;
    if (!detect_word(smooth, labels, slots, t, x, y, cap, f, word, one, slot)) continue;
    if (!f || slot < 0) continue;
    const int lead = __ffsll((long long)word) - 1;
    if (one && lane != lead) continue;
    const int c = dirs[(size_t)(first + slot) * 2], s = dirs[(size_t)(first + slot) * 2 + 1];
    if (c == 0 && s == 0) continue;
    int* row = table + (size_t)(first + slot) * 4;
    const int Y = 2 * y + 1, Xa = 2 * x + 1;
    if (one) {      // one root: U2 and V2 are linear in x, so the word's first and last set bit give its extremes
      const int Xb = 2 * (t.x0 + 63 - __clzll((long long)word)) + 1;
      const int Ua = c * Xa + s * Y, Ub = c * Xb + s * Y, Va = c * Y - s * Xa, Vb = c * Y - s * Xb;
      atomicMax(&row[0], -min(Ua, Ub));
      atomicMax(&row[1], max(Ua, Ub));
      atomicMax(&row[2], -min(Va, Vb));
      atomicMax(&row[3], max(Va, Vb));
    } else {
      const int U = c * Xa + s * Y, V = c * Y - s * Xa;
      atomicMax(&row[0], -U);
      atomicMax(&row[1], U);
      atomicMax(&row[2], -V);
      atomicMax(&row[3], V);
    }
  }
}

// Bowed lines (utils/detect.py, stage b of the curved recipe).  bins: int32 (table_rows, 3) per component [x0, w, n]: its box's first
// column and width and the number of its bins, n = 0: passed over.  Bin i begins at e_i = x0 + i w / n, the bin of column x is
// ((x - x0 + 1) n - 1) / w, the greatest i with e_i <= x.  table: int32 (table_rows, DETECT_BINS, 4) [max -y, max y, count, sum y] per
// component and bin, initialised by the entry point (the extrema to a value below every y and -y, the sums to zero).  A component has
// at most 64 * 1024 pixels in a bin and y < 1024, so count <= 2^16 and sum y < 2^26: 32-bit atomics suffice.  A row of bins that does
// not describe its component (x outside [x0, x0 + w), n outside 1 .. DETECT_BINS) adds nothing: no index is taken from data unchecked.
constexpr int DETECT_BINS = 16;

__global__ void __launch_bounds__(DT_THREADS)
k_detect_profile(const unsigned char* __restrict__ smooth, const int* __restrict__ labels, long map_px, const long long* __restrict__ items,
                 int B, const int* __restrict__ tiles, const long long* __restrict__ slices, const int* __restrict__ slots,
                 const int* __restrict__ bins, int* __restrict__ table, long table_rows) {
  DetTile t;
  if (!detect_tile(items, B, tiles, -1, map_px, t)) return;
  long long first, cap;
  if (!detect_slice(slices, t.b, table_rows, first, cap)) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = t.x0 + lane;
  for (int k = 0; k < DT_WAVE_ROWS; ++k) {
    const int y = t.y0 + wave * DT_WAVE_ROWS + k;
    bool f, one;
    u64 word;
    int slot;
    if (!detect_word(smooth, labels, slots, t, x, y, cap, f, word, one, slot)) continue;
    if (!f || slot < 0) continue;
    const int* q = bins + (size_t)(first + slot) * 3;
    const int cx0 = q[0], cw = q[1], n = q[2];
    if (n < 1 || n > DETECT_BINS || cw < n || cw > DETECT_MAP_SIDE || x < cx0 || x - cx0 >= cw) continue;
    const int i = ((x - cx0 + 1) * n - 1) / cw;      // 0 .. n - 1, since 0 <= x - cx0 < cw
    int* row = table + ((size_t)(first + slot) * DETECT_BINS + i) * 4;
    if (one) {
      // one root: the pixels of the word that share this lane's bin lie in the lanes [e_i, e_{i+1}) - t.x0; the first of them sends the
      // segment's update (every pixel of the word has this y).  A word may span several bins and a bin several words.
      const int lo = max(cx0 + i * cw / n - t.x0, 0), hi = min(cx0 + (i + 1) * cw / n - t.x0, DT_W);      // lo <= lane < hi
      const u64 seg = word & ((hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1));
      if (lane != __ffsll((long long)seg) - 1) continue;
      const int n_px = __popcll(seg);
      atomicMax(&row[0], -y);
      atomicMax(&row[1], y);
      atomicAdd(&row[2], n_px);
      atomicAdd(&row[3], y * n_px);
    } else {
      atomicMax(&row[0], -y);
      atomicMax(&row[1], y);
      atomicAdd(&row[2], 1);
      atomicAdd(&row[3], y);
    }
  }
}

int detect_check(const long long* items_host, int B, long packed_bytes, long map_px) {
  for (int b = 0; b < B; ++b)
    if (!detect_item_ok(items_host + (size_t)b * DETECT_ITEM_WORDS, packed_bytes, map_px)) return 0;
  return 1;
}

}  // namespace

extern "C" {

int dpmn_detect_gradient_u8(const unsigned char* packed, long packed_bytes, const long long* items, const long long* items_host, int B,
                            const int* tiles, int n_tiles, unsigned char* g, long map_px, unsigned* hist, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed && items && items_host && hist, "detect_gradient: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles >= 0 && (tiles || n_tiles == 0) && map_px >= 0 && (g || map_px == 0), "detect_gradient: bad sizes");
  DPMN_REQUIRE(packed_bytes > 0 && detect_check(items_host, B, packed_bytes, map_px),
               "detect_gradient: a photo does not fit the buffers, has a side outside 1 .. 8192 or a working map that is not its own");
  if (hipMemsetAsync(hist, 0, (size_t)B * 256 * sizeof(unsigned), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "detect_gradient: hipMemsetAsync failed");
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_detect_grad, dim3((unsigned)n_tiles), dim3(DT_THREADS), 0, as_stream(stream), packed, packed_bytes, items, B, tiles, g,
                       map_px, hist);
    DPMN_CHECK_LAUNCH();
  }
  return DPMN_OK;
}

int dpmn_detect_label_i32(const unsigned char* g, long map_px, const long long* items, const long long* items_host, int B, const int* tiles,
                          int n_tiles, const int* thresholds, int gap, int vgap, unsigned char* tmp, unsigned char* smooth, int* labels,
                          dpmn_stream_t stream) {
  if (n_tiles == 0) return DPMN_OK;
  DPMN_REQUIRE(g && items && items_host && tiles && thresholds && tmp && smooth && labels, "detect_label: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles > 0 && map_px > 0, "detect_label: bad sizes");
  DPMN_REQUIRE(gap >= 1 && gap <= DETECT_MAX_GAP && vgap >= 1 && vgap <= DETECT_MAX_GAP, "detect_label: gap and vgap must be 1 .. 64");
  DPMN_REQUIRE(detect_check(items_host, B, -1, map_px), "detect_label: a working map does not fit the buffers or is not its photo's");
  const dim3 grid((unsigned)n_tiles), block(DT_THREADS);
  hipLaunchKernelGGL(k_detect_hsmooth, grid, block, 0, as_stream(stream), g, map_px, items, B, tiles, thresholds, gap, tmp);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_detect_vsmooth, grid, block, 0, as_stream(stream), (const unsigned char*)tmp, map_px, items, B, tiles, vgap, smooth, labels);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_detect_union, grid, block, 0, as_stream(stream), (const unsigned char*)smooth, labels, map_px, items, B, tiles);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

// Word 7 of every item is the running sum of the photos' cell counts and the sums end at n_cells: the table has exactly one owner per
// entry, and k_detect_cell_otsu may look a cell's photo up by halving.
static int detect_cells_check(const long long* items_host, int B, int C, long n_cells) {
  long long at = 0;
  for (int b = 0; b < B; ++b) {
    const long long* p = items_host + (size_t)b * DETECT_ITEM_WORDS;
    if (p[7] != at) return 0;
    at += (long long)detect_cells((int)p[4], C) * detect_cells((int)p[5], C);
  }
  return at == n_cells;
}

int dpmn_detect_cell_otsu_i32(const unsigned char* g, long map_px, const long long* items, const long long* items_host, int B, int cell,
                              int floor, int* table, long n_cells, dpmn_stream_t stream) {
  DPMN_REQUIRE(items && items_host, "detect_cell_otsu: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && map_px >= 0 && n_cells >= 0 && n_cells <= 0x7fffffffL, "detect_cell_otsu: bad sizes");
  DPMN_REQUIRE(cell >= 32 && cell <= DETECT_MAP_SIDE && floor >= 1 && floor <= 255, "detect_cell_otsu: the cell side must be 32 .. 1024 and the floor 1 .. 255");
  DPMN_REQUIRE(detect_check(items_host, B, -1, map_px), "detect_cell_otsu: a working map does not fit the buffers or is not its photo's");
  DPMN_REQUIRE(detect_cells_check(items_host, B, cell, n_cells), "detect_cell_otsu: the items' cell offsets are not the running sum of their cell counts");
  if (n_cells == 0) return DPMN_OK;
  DPMN_REQUIRE(g && table && map_px > 0, "detect_cell_otsu: null pointer");
  hipLaunchKernelGGL(k_detect_cell_otsu, dim3((unsigned)n_cells), dim3(DT_THREADS), 0, as_stream(stream), g, map_px, items, B, cell, floor, table,
                     n_cells);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_detect_label_local_i32(const unsigned char* g, long map_px, const long long* items, const long long* items_host, int B,
                                const int* tiles, int n_tiles, const int* table, long n_cells, int cell, int gap, int vgap, unsigned char* tmp,
                                unsigned char* smooth, int* labels, int* tmap, dpmn_stream_t stream) {
  if (n_tiles == 0) return DPMN_OK;
  DPMN_REQUIRE(g && items && items_host && tiles && table && tmp && smooth && labels, "detect_label_local: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles > 0 && map_px > 0 && n_cells > 0, "detect_label_local: bad sizes");
  DPMN_REQUIRE(gap >= 1 && gap <= DETECT_MAX_GAP && vgap >= 1 && vgap <= DETECT_MAX_GAP, "detect_label_local: gap and vgap must be 1 .. 64");
  DPMN_REQUIRE(cell >= 32 && cell <= DETECT_MAP_SIDE, "detect_label_local: the cell side must be 32 .. 1024");
  DPMN_REQUIRE(detect_check(items_host, B, -1, map_px), "detect_label_local: a working map does not fit the buffers or is not its photo's");
  DPMN_REQUIRE(detect_cells_check(items_host, B, cell, n_cells), "detect_label_local: the items' cell offsets are not the running sum of their cell counts");
  const dim3 grid((unsigned)n_tiles), block(DT_THREADS);
  hipLaunchKernelGGL(k_detect_hsmooth_local, grid, block, 0, as_stream(stream), g, map_px, items, B, tiles, table, n_cells, cell, gap, tmp, tmap);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_detect_vsmooth, grid, block, 0, as_stream(stream), (const unsigned char*)tmp, map_px, items, B, tiles, vgap, smooth, labels);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_detect_union, grid, block, 0, as_stream(stream), (const unsigned char*)smooth, labels, map_px, items, B, tiles);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_detect_stats_i32(const unsigned char* smooth, int* labels, long map_px, const long long* items, const long long* items_host, int B,
                          const int* tiles, int n_tiles, const long long* slices, const long long* slices_host, int* counts, int* slots,
                          int* table, long table_rows, dpmn_stream_t stream) {
  DPMN_REQUIRE(items && items_host && slices && slices_host && counts, "detect_stats: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles >= 0 && map_px >= 0 && table_rows >= 0, "detect_stats: bad sizes");
  DPMN_REQUIRE(n_tiles == 0 || (smooth && labels && tiles && slots && map_px > 0), "detect_stats: null pointer");
  DPMN_REQUIRE(table || table_rows == 0, "detect_stats: null table");
  DPMN_REQUIRE(detect_check(items_host, B, -1, map_px), "detect_stats: a working map does not fit the buffers or is not its photo's");
  for (int b = 0; b < B; ++b) {
    const long long first = slices_host[(size_t)b * 2], cap = slices_host[(size_t)b * 2 + 1];
    DPMN_REQUIRE(first >= 0 && cap >= 0 && first <= table_rows - cap, "detect_stats: a photo's rows leave the table");
  }
  if (hipMemsetAsync(counts, 0, (size_t)B * sizeof(int), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "detect_stats: hipMemsetAsync failed");
  if (n_tiles == 0) return DPMN_OK;
  const dim3 grid((unsigned)n_tiles), block(DT_THREADS);
  hipLaunchKernelGGL(k_detect_roots, grid, block, 0, as_stream(stream), (const int*)labels, map_px, items, B, tiles, slices, counts, slots, table,
                     table_rows);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_detect_stats, grid, block, 0, as_stream(stream), smooth, labels, map_px, items, B, tiles, slices, (const int*)slots, table,
                     table_rows);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

// The checks that the two oriented entry points share with dpmn_detect_stats_i32.
static int detect_oriented_check(const void* smooth, const void* labels, long map_px, const long long* items,
                                 const long long* items_host, int B, const int* tiles, int n_tiles, const long long* slices,
                                 const long long* slices_host, const void* slots, const void* table, long table_rows) {
  DPMN_REQUIRE(items && items_host && slices && slices_host, "detect_oriented: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles >= 0 && map_px >= 0 && table_rows >= 0, "detect_oriented: bad sizes");
  DPMN_REQUIRE(n_tiles == 0 || (smooth && labels && tiles && slots && map_px > 0), "detect_oriented: null pointer");
  DPMN_REQUIRE(table || table_rows == 0, "detect_oriented: null table");
  DPMN_REQUIRE(detect_check(items_host, B, -1, map_px), "detect_oriented: a working map does not fit the buffers or is not its photo's");
  for (int b = 0; b < B; ++b) {
    const long long first = slices_host[(size_t)b * 2], cap = slices_host[(size_t)b * 2 + 1];
    DPMN_REQUIRE(first >= 0 && cap >= 0 && first <= table_rows - cap, "detect_oriented: a photo's rows leave the table");
  }
  return DPMN_OK;
}

int dpmn_detect_moments_i64(const unsigned char* smooth, const int* labels, long map_px, const long long* items, const long long* items_host,
                            int B, const int* tiles, int n_tiles, const long long* slices, const long long* slices_host, const int* slots,
                            long long* table, long table_rows, dpmn_stream_t stream) {
  const int rc = detect_oriented_check(smooth, labels, map_px, items, items_host, B, tiles, n_tiles, slices, slices_host,
                                       slots, table, table_rows);
  if (rc != DPMN_OK) return rc;
  if (table_rows > 0 && hipMemsetAsync(table, 0, (size_t)table_rows * 5 * sizeof(long long), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "detect_moments: hipMemsetAsync failed");
  if (n_tiles == 0 || table_rows == 0) return DPMN_OK;
  hipLaunchKernelGGL(k_detect_moments, dim3((unsigned)n_tiles), dim3(DT_THREADS), 0, as_stream(stream), smooth, labels, map_px, items, B, tiles,
                     slices, slots, (u64*)table, table_rows);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_detect_extents_i32(const unsigned char* smooth, const int* labels, long map_px, const long long* items, const long long* items_host,
                            int B, const int* tiles, int n_tiles, const long long* slices, const long long* slices_host, const int* slots,
                            const int* dirs, int* table, long table_rows, dpmn_stream_t stream) {
  const int rc = detect_oriented_check(smooth, labels, map_px, items, items_host, B, tiles, n_tiles, slices, slices_host,
                                       slots, table, table_rows);
  if (rc != DPMN_OK) return rc;
  DPMN_REQUIRE(dirs || table_rows == 0, "detect_extents: null directions");
  if (table_rows > 0 && hipMemsetAsync(table, 0x80, (size_t)table_rows * 4 * sizeof(int), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "detect_extents: hipMemsetAsync failed");
  if (n_tiles == 0 || table_rows == 0) return DPMN_OK;
  hipLaunchKernelGGL(k_detect_extents, dim3((unsigned)n_tiles), dim3(DT_THREADS), 0, as_stream(stream), smooth, labels, map_px, items, B, tiles,
                     slices, slots, dirs, table, table_rows);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_detect_profile_i32(const unsigned char* smooth, const int* labels, long map_px, const long long* items, const long long* items_host,
                            int B, const int* tiles, int n_tiles, const long long* slices, const long long* slices_host, const int* slots,
                            const int* bins, int* table, long table_rows, dpmn_stream_t stream) {
  const int rc = detect_oriented_check(smooth, labels, map_px, items, items_host, B, tiles, n_tiles, slices, slices_host,
                                       slots, table, table_rows);
  if (rc != DPMN_OK) return rc;
  DPMN_REQUIRE(bins || table_rows == 0, "detect_profile: null bins");
  DPMN_REQUIRE(table_rows <= 0x7fffffffL / DETECT_BINS, "detect_profile: too many rows");
  if (table_rows > 0) {
    // per bin 16 bytes: the two extrema every byte 0x80 (below every y and -y, so that atomicMax does it), the two sums zero
    const size_t n_bins = (size_t)table_rows * DETECT_BINS;
    if (hipMemsetAsync(table, 0, n_bins * 4 * sizeof(int), as_stream(stream)) != hipSuccess ||
        hipMemset2DAsync(table, 4 * sizeof(int), 0x80, 2 * sizeof(int), n_bins, as_stream(stream)) != hipSuccess)
      return dpmn_set_error(DPMN_ERR_LAUNCH, "detect_profile: hipMemsetAsync failed");
  }
  if (n_tiles == 0 || table_rows == 0) return DPMN_OK;
  hipLaunchKernelGGL(k_detect_profile, dim3((unsigned)n_tiles), dim3(DT_THREADS), 0, as_stream(stream), smooth, labels, map_px, items, B, tiles,
                     slices, slots, bins, table, table_rows);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
