// The overlap of detected and ground-truth regions in samples (include/dpmn_hip.h "detect_eval.hip"; utils/detect_eval.py is the
// definition; main.py --demo_eval).  4 x 4 samples per pixel at x = 200 c + 100, y = 200 m + 100 in units of 1 / 800 pixel, even-odd
// rule, integers only.  A block takes DE_THREADS sample rows of one item (a region: its area; a pair: the intersection), one row per
// thread, with the item's edges in LDS (every thread walks the same edge at the same time: broadcast reads).  On its row a thread
// turns every crossing edge into its break t = ceil((crossing - 100) / 200) -- the edge lies right of exactly the sample columns
// c < t -- keeps the breaks sorted in its own LDS column, and counts by subtraction: [t0, t1), [t2, t3), ... are the inside columns.
// The one division per crossing is a double quotient corrected by an exact integer remainder (numerator < 2^51, so both operands
// are exact doubles and the estimate is off by one at most): no 64-bit integer division.  A row with more than DE_SLOTS crossings
// of a region tests its samples one by one with the definition's cross product.  Counts are reduced in the wave, then across the
// block's waves in LDS, and one 64-bit atomic per block adds them to the item's count.
#include <algorithm>
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int DE_THREADS = 128;       // sample rows per block
constexpr int DE_MAX_POINTS = 64;
constexpr int DE_SLOTS = 8;           // sorted breaks a thread keeps per region (even)
constexpr int DE_STEP = 200, DE_SUB = 4, DE_MAX_BOX = 16385;
constexpr int DE_REGION_WORDS = 8;

struct DeRegion {
  int off, n, x0, y0, x1, y1;
};

__host__ __device__ inline bool de_region_ok(const int* p, long n_verts, DeRegion& g) {
  g.off = p[0]; g.n = p[1]; g.x0 = p[2]; g.y0 = p[3]; g.x1 = p[4]; g.y1 = p[5];
  return g.off >= 0 && g.n >= 4 && g.n <= DE_MAX_POINTS && (long)g.off + g.n <= n_verts && g.x0 >= -DE_MAX_BOX && g.y0 >= -DE_MAX_BOX &&
         g.x1 <= DE_MAX_BOX && g.y1 <= DE_MAX_BOX && g.x0 <= g.x1 && g.y0 <= g.y1;
}

// ceil(((x0 - 100) dy + (py - y0) dx) / (200 dy)), dy made positive
__device__ __forceinline__ int de_break(const int4 e, int py) {
  long long dy = (long long)e.w - e.y;
  long long num = (long long)(e.x - DE_STEP / 2) * dy + (long long)(py - e.y) * ((long long)e.z - e.x);
  if (dy < 0) { dy = -dy; num = -num; }
  const long long den = DE_STEP * dy;
  long long q = (long long)floor((double)num / (double)den);
  long long r = num - q * den;
  if (r < 0) { q -= 1; r += den; }
  else if (r >= den) { q += 1; r -= den; }
  return (int)(q + (r > 0 ? 1 : 0));
}

// the sorted, clamped breaks of row py into slots[j * DE_THREADS]; -1: more than DE_SLOTS crossings
__device__ __forceinline__ int de_gather(const int4* __restrict__ e, int n, int py, int c0, int c1, int* slots) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const int4 v = e[i];
    if ((v.y > py) == (v.w > py)) continue;
    if (k == DE_SLOTS) return -1;
    const int t = min(max(de_break(v, py), c0), c1);
    int j = k;
    while (j > 0 && slots[(j - 1) * DE_THREADS] > t) {
      slots[j * DE_THREADS] = slots[(j - 1) * DE_THREADS];
      --j;
    }
    slots[j * DE_THREADS] = t;
    ++k;
  }
  return k;
}

// the definition's test of one sample
__device__ __forceinline__ bool de_inside(const int4* __restrict__ e, int n, int px, int py) {
  bool in = false;
  for (int i = 0; i < n; ++i) {
    const int4 v = e[i];
    if ((v.y > py) == (v.w > py)) continue;
    const long long dy = (long long)v.w - v.y;
    const long long cross = ((long long)v.z - v.x) * (py - v.y) - ((long long)px - v.x) * dy;
    in ^= dy > 0 ? cross > 0 : cross < 0;      // (cross == 0, the sample on the edge: not to the right)
  }
  return in;
}

__device__ __forceinline__ void de_stage(const int* __restrict__ verts, const DeRegion& g, int4* e) {
  for (int i = (int)threadIdx.x; i < g.n; i += DE_THREADS) {
    const int j = i + 1 == g.n ? 0 : i + 1;
    const int* a = verts + ((size_t)g.off + i) * 2;
    const int* b = verts + ((size_t)g.off + j) * 2;
    e[i] = make_int4(a[0], a[1], b[0], b[1]);
  }
}

template <bool PAIR>
__global__ void __launch_bounds__(DE_THREADS)
k_region_counts(const int* __restrict__ verts, long n_verts, const int* __restrict__ regions, int n_regions, const int* __restrict__ pairs,
                int n_pairs, const int* __restrict__ units, u64* __restrict__ out) {
  __shared__ int4 edges[2][DE_MAX_POINTS];
  __shared__ int slots[2][DE_SLOTS][DE_THREADS];
  __shared__ u64 part[DE_THREADS / 64];
  const int tid = (int)threadIdx.x;
  const int item = units[(size_t)blockIdx.x * 2], first = units[(size_t)blockIdx.x * 2 + 1];
  if (item < 0 || item >= (PAIR ? n_pairs : n_regions) || first < 0) return;      // (block-uniform, as every return below)
  const int ra = PAIR ? pairs[(size_t)item * 2] : item, rb = PAIR ? pairs[(size_t)item * 2 + 1] : item;
  if (ra < 0 || ra >= n_regions || rb < 0 || rb >= n_regions) return;
  DeRegion a, b;
  if (!de_region_ok(regions + (size_t)ra * DE_REGION_WORDS, n_verts, a)) return;
  if (!de_region_ok(regions + (size_t)rb * DE_REGION_WORDS, n_verts, b)) return;
  const int bx0 = max(a.x0, b.x0), by0 = max(a.y0, b.y0), bx1 = min(a.x1, b.x1), by1 = min(a.y1, b.y1);
  if (bx0 >= bx1 || by0 >= by1) return;
  const int rows = DE_SUB * (by1 - by0);
  if (first >= rows) return;
  de_stage(verts, a, edges[0]);
  if (PAIR) de_stage(verts, b, edges[1]);
  __syncthreads();
  u64 cnt = 0;
  const int row = first + tid;
  if (row < rows) {
    const int py = DE_STEP * (DE_SUB * by0 + row) + DE_STEP / 2, c0 = DE_SUB * bx0, c1 = DE_SUB * bx1;
    int* sa = &slots[0][0][tid];
    int* sb = &slots[1][0][tid];
    const int ka = de_gather(edges[0], a.n, py, c0, c1, sa);
    const int kb = PAIR ? de_gather(edges[1], b.n, py, c0, c1, sb) : 0;
    if (ka < 0 || kb < 0) {
      for (int c = c0; c < c1; ++c) {
        const int px = DE_STEP * c + DE_STEP / 2;
        if (de_inside(edges[0], a.n, px, py) && (!PAIR || de_inside(edges[1], b.n, px, py))) ++cnt;
      }
    } else if (!PAIR) {
      for (int j = 0; j + 1 < ka; j += 2) cnt += (u64)(sa[(j + 1) * DE_THREADS] - sa[j * DE_THREADS]);
    } else {
      int i = 0, j = 0;
      while (i + 1 < ka && j + 1 < kb) {
        const int a1 = sa[(i + 1) * DE_THREADS], b1 = sb[(j + 1) * DE_THREADS];
        const int d = min(a1, b1) - max(sa[i * DE_THREADS], sb[j * DE_THREADS]);
        if (d > 0) cnt += (u64)d;
        if (a1 < b1) i += 2; else j += 2;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += xshfl_v(cnt, o);
  if ((tid & 63) == 0) part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    u64 total = 0;
#pragma unroll
    for (int w = 0; w < DE_THREADS / 64; ++w) total += part[w];
    if (total) atomicAdd(out + item, total);
  }
}

// the tables of a call in HOST memory: every region, pair and unit names what exists
int de_check(long n_verts, const int* regions_host, int n_regions, const int* pairs_host, int n_pairs, const int* units_host, int n_units) {
  DeRegion g, h;
  for (int r = 0; r < n_regions; ++r)
    if (!de_region_ok(regions_host + (size_t)r * DE_REGION_WORDS, n_verts, g)) return 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int a = pairs_host[(size_t)p * 2], b = pairs_host[(size_t)p * 2 + 1];
    if (a < 0 || a >= n_regions || b < 0 || b >= n_regions) return 0;
  }
  const int n_items = pairs_host ? n_pairs : n_regions;
  for (int u = 0; u < n_units; ++u) {
    const int item = units_host[(size_t)u * 2], first = units_host[(size_t)u * 2 + 1];
    if (item < 0 || item >= n_items || first < 0 || first % DE_THREADS) return 0;
    const int ra = pairs_host ? pairs_host[(size_t)item * 2] : item, rb = pairs_host ? pairs_host[(size_t)item * 2 + 1] : item;
    de_region_ok(regions_host + (size_t)ra * DE_REGION_WORDS, n_verts, g);
    de_region_ok(regions_host + (size_t)rb * DE_REGION_WORDS, n_verts, h);
    if (first >= DE_SUB * (std::min(g.y1, h.y1) - std::max(g.y0, h.y0))) return 0;
  }
  return 1;
}

}  // namespace

extern "C" {

int dpmn_region_block(void) { return DE_THREADS; }

int dpmn_region_area_u64(const int* verts, long n_verts, const int* regions, const int* regions_host, int n_regions, const int* units,
                         const int* units_host, int n_units, u64* area, dpmn_stream_t stream) {
  DPMN_REQUIRE(n_regions >= 0 && n_units >= 0 && n_verts >= 0, "region_area: bad sizes");
  if (n_regions == 0) return DPMN_OK;
  DPMN_REQUIRE(verts && regions && regions_host && area && ((units && units_host) || n_units == 0), "region_area: null pointer");
  DPMN_REQUIRE(de_check(n_verts, regions_host, n_regions, nullptr, 0, units_host, n_units),
               "region_area: a region leaves the vertex table, has a box beyond 16385 pixels or not 4 .. 64 points, or a unit names no row");
  if (hipMemsetAsync(area, 0, (size_t)n_regions * sizeof(u64), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "region_area: hipMemsetAsync failed");
  if (n_units == 0) return DPMN_OK;
  hipLaunchKernelGGL(k_region_counts<false>, dim3((unsigned)n_units), dim3(DE_THREADS), 0, as_stream(stream), verts, n_verts, regions,
                     n_regions, (const int*)nullptr, 0, units, area);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_region_inter_u64(const int* verts, long n_verts, const int* regions, const int* regions_host, int n_regions, const int* pairs,
                          const int* pairs_host, int n_pairs, const int* units, const int* units_host, int n_units, u64* inter,
                          dpmn_stream_t stream) {
  DPMN_REQUIRE(n_regions >= 0 && n_pairs >= 0 && n_units >= 0 && n_verts >= 0, "region_inter: bad sizes");
  if (n_pairs == 0) return DPMN_OK;
  DPMN_REQUIRE(verts && regions && regions_host && pairs && pairs_host && inter && ((units && units_host) || n_units == 0),
               "region_inter: null pointer");
  DPMN_REQUIRE(de_check(n_verts, regions_host, n_regions, pairs_host, n_pairs, units_host, n_units),
               "region_inter: a region leaves the vertex table, has a box beyond 16385 pixels or not 4 .. 64 points, or a pair or a "
               "unit names nothing");
  if (hipMemsetAsync(inter, 0, (size_t)n_pairs * sizeof(u64), as_stream(stream)) != hipSuccess)
    return dpmn_set_error(DPMN_ERR_LAUNCH, "region_inter: hipMemsetAsync failed");
  if (n_units == 0) return DPMN_OK;
  hipLaunchKernelGGL(k_region_counts<true>, dim3((unsigned)n_units), dim3(DE_THREADS), 0, as_stream(stream), verts, n_verts, regions,
                     n_regions, pairs, n_pairs, units, inter);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
