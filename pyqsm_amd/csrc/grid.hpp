// grid.hpp — uniform cell grid over a point cloud in HBM: the binning step that
// the eps-neighbourhood (DBSCAN) and kNN kernels share.
//
// Layout: cells are row-major with x fastest and carry a one-cell empty border,
// so the 3x3x3 stencil of any point is nine contiguous runs of the sorted point
// array: [start[row + cx - 1], start[row + cx + 2]) for each of the 9 (y,z) rows.
// Points are counting-sorted by cell into SoA coordinate arrays (coalesced,
// 8-byte loads per lane).
//
// Two forms of the directory `start`. build_grid (kNN, radius, features, normals, adjacency) keeps the
// dense array, 4 bytes per cell. DBSCAN's octant binning keeps a RANKED directory instead (CellDir
// below): an occupancy bitmap and a slot base per 32 cells plus the begins of the occupied cells
// only, because a forest's grid is 99.6 % air and the dense array was a quarter of the binning's
// traffic and far larger than an L2.
#pragma once
#include "common.hpp"

namespace pyqsm {

// ---- the ranked cell directory ----------------------------------------------------------------
// Cell ids 32 w .. 32 w + 31 share words[w]: bit i says cell 32 w + i holds a point, and the begins
// of the word's occupied cells lie at slots[base], slots[base + 1], ... in id order, followed by the
// begin of the next occupied cell after them. So
//   occupied(c) = (words[c >> 5].bits >> (c & 31)) & 1
//   begin(c)    = slots[w.base + popc(w.bits & ((1u << (c & 31)) - 1))],   w = words[c >> 5]
// and for every 0 <= c <= ncell, begin(c) is what a dense start[c] holds: the number of points in
// cells with id < c (for an empty cell the begin of the next occupied one; begin(ncell) = n). The
// count of a cell is begin(c + 1) - begin(c), and the stencil runs [begin(row - 1), begin(row + 2))
// and wave_tile's linear intervals read as from the dense array. Any producer that keeps this
// contract will do (k_bk_sort per bucket, k_dir_from_dense per word); consumers know only CellDir.
struct alignas(8) DirWord {
  uint32_t bits, base;
};
// (Kernels take the two arrays as `const ... __restrict__` parameters of their own and build the CellDir
// in their first line: only then does the compiler know the tables as read-only, and a look-up at a
// wave-uniform cell stays on the scalar path. With the struct as the parameter k_core_tiled's eighteen
// bounds became vector loads: 58 VGPRs instead of 42.)
struct CellDir {
  const DirWord* words;
  const int32_t* slots;
  __device__ __forceinline__ static int slot_of(const DirWord w, int c) {
    return int(w.base) + __popc(w.bits & ((1u << (c & 31)) - 1u));
  }
  __device__ __forceinline__ int begin(int c) const { return slots[slot_of(words[c >> 5], c)]; }
  // begin() of N cells: the word loads side by side, then the slot loads side by side (two round
  // trips, not N chains)
  template <int N>
  __device__ __forceinline__ void begins(const int (&c)[N], int (&out)[N]) const {
    DirWord w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = words[c[i] >> 5];
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = slots[slot_of(w[i], c[i])];
  }
};

struct DevGrid {
  double minx, miny, minz;
  double inv_cell;
  double cell;
  int nx, ny, nz;        // including the border cells
  int64_t ncell;         // nx*ny*nz
  int32_t* start;        // [ncell + 1] first sorted position of each cell (null from the two-level octant binning)
  // the ranked directory (DBSCAN's octant binning only; see CellDir)
  DirWord* dir_words = nullptr;
  int32_t* dir_slots = nullptr;
  int32_t* order;        // [n] sorted position -> original index
  int32_t* cell_of;      // [n] cell id of each sorted position
  double *sx, *sy, *sz;  // [n] sorted coordinates (fp64 storage)
  // [n] sorted coordinates as one 16-byte (x, y, z, 0) fp32 record per point, INSTEAD of sx / sy /
  // sz (those are then null): only when every input coordinate is exactly representable in fp32
  // (cloud_bbox's flag), so that double(p4[q].x) IS the input value and every fp64 predicate
  // evaluated on it is bit-identical. Half the bytes, and a gather touches one line, not three.
  float4* p4 = nullptr;
  // build_grid only: per block of its counting pass, the points that were the first of their
  // cell — their sum is the number of occupied cells (count_occupied), without a pass over
  // the ncell-long start array
  int32_t* occ_part = nullptr;
  int occ_blocks = 0;
};

// ---- the grid's geometry, as kernels take it by value -----------------------------------------
struct GridParams {
  double minx, miny, minz, inv_cell;
  int nx, ny, nz;
};
inline CellDir cell_dir(const DevGrid& g) { return CellDir{g.dir_words, g.dir_slots}; }
inline GridParams grid_params(const DevGrid& g) { return GridParams{g.minx, g.miny, g.minz, g.inv_cell, g.nx, g.ny, g.nz}; }

// The cell a point is binned into, and the cell every lookup of it must use: interior cells are
// 1 .. n-2; the clamp guards the max-boundary point and puts points outside the grid's box into its
// outermost cells — clamped in double, so that a point a light year away does not overflow the int.
// A clamp moves no two points further apart, so whatever lies within a cell edge of a point outside
// the box still sits in the 27 cells around its clamped cell.
__device__ __forceinline__ void clamped_cell(const GridParams& g, double x, double y, double z, int* cx, int* cy,
                                             int* cz) {
  const double fx = floor((x - g.minx) * g.inv_cell), fy = floor((y - g.miny) * g.inv_cell),
               fz = floor((z - g.minz) * g.inv_cell);
  *cx = int(fmin(fmax(fx, 0.0), double(g.nx - 3))) + 1;
  *cy = int(fmin(fmax(fy, 0.0), double(g.ny - 3))) + 1;
  *cz = int(fmin(fmax(fz, 0.0), double(g.nz - 3))) + 1;
}

__device__ __forceinline__ int cell_index(const GridParams& g, double x, double y, double z) {
  int cx, cy, cz;
  clamped_cell(g, x, y, z, &cx, &cy, &cz);
  return (cz * g.ny + cy) * g.nx + cx;
}

// The 27-cell stencil of a point as nine runs [qb[w], qe[w]) of sorted positions, one per (y,z) row
// (empty for rows outside the grid).
struct StencilRuns {
  int qb[9], qe[9];
};

__device__ __forceinline__ void point_stencil_runs(const GridParams& g, const int32_t* __restrict__ start, double x,
                                                   double y, double z, StencilRuns* rr) {
  int cx, cy, cz;
  clamped_cell(g, x, y, z, &cx, &cy, &cz);
  int w = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy, ++w) {
      const int zz = cz + dz, yy = cy + dy;
      rr->qb[w] = rr->qe[w] = 0;
      if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny) continue;
      const int x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
      const int row = (zz * g.ny + yy) * g.nx;
      rr->qb[w] = start[row + x0];
      rr->qe[w] = start[row + x1 + 1];
    }
}

// Builds the grid for n points (f64 [n,3], device) with cells of at least
// `min_cell` edge (the edge is doubled until the dense grid has at most
// `max_cells` cells). All arrays come from the context arena. Synchronises the
// stream once (bounding box read-back). Fails with PYQSM_EINVAL on non-finite
// coordinates.
// `bbox` (min xyz, max xyz), when given, skips the bounding-box pass. `f32_records`: the caller
// knows (cloud_bbox) that every coordinate is fp32-representable and reads the grid through
// on_coords(): the sorted points are then kept as g->p4 instead of g->sx / sy / sz.
int build_grid(Ctx* c, const double* xyz, int64_t n, double min_cell, int64_t max_cells,
               DevGrid* g, const double* bbox = nullptr, bool f32_records = false);

// Bounding box of the cloud (one reduction kernel, a one-block fold, a 56-byte read-back).
// *all_f32 (optional): every coordinate is exactly representable in fp32. zero_buf / zero_n
// (optional): ints the reduction kernel clears on the way (saves the caller a memset launch).
int cloud_bbox(Ctx* c, const double* xyz, int64_t n, double mn[3], double mx[3], bool* all_f32 = nullptr,
               int32_t* zero_buf = nullptr, int zero_n = 0);
// Shrinks box (min xyz, max xyz) to the part of the cloud that is left when at most `budget`
// points in sparse tails are given up (they clamp into the outermost cells of a grid built over
// the box); *outside = how many the last cut gave up (0: box unchanged).
int robust_box(Ctx* c, const double* xyz, int64_t n, int budget, double box[6], int64_t* outside);

// Mean number of points per occupied cell for a grid of edge `cell` over `box`
// (count-only pass on a grid of at most 4 M cells; the edge is doubled to fit and
// the edge actually used is returned). Synchronises.
int probe_occupancy(Ctx* c, const double* xyz, int64_t n, const double box[6], double cell,
                    double* cell_used, double* per_cell);

struct Stencil {
  int nx, nxy;
};

// ---- how the neighbourhood kernels read a sorted point ------------------------------------
// Both forms hand out fp64 values and evaluate d2 = ((dx*dx) + dy*dy) + dz*dz with separately
// rounded products (the library is built with -ffp-contract=off): the predicate does not know
// how the coordinates were stored.
__device__ __forceinline__ double sqdist3(double ax, double ay, double az, double bx, double by, double bz) {
  const double t0 = ax - bx, t1 = ay - by, t2 = az - bz;
  double d = t0 * t0;
  d = d + t1 * t1;
  d = d + t2 * t2;
  return d;
}
struct CoordsF64 {
  const double *x, *y, *z;
  __device__ __forceinline__ void get(int q, double& a, double& b, double& c) const {
    a = x[q];
    b = y[q];
    c = z[q];
  }
  __device__ __forceinline__ double d2(int q, double px, double py, double pz) const {
    return sqdist3(px, py, pz, x[q], y[q], z[q]);
  }
  __device__ __forceinline__ double d2(int a, int q) const {
    return sqdist3(x[a], y[a], z[a], x[q], y[q], z[q]);
  }
  // core flag of a sorted point: lives in its own byte array for this storage form
  __device__ __forceinline__ void mark_core(int, bool) const {}
  __device__ __forceinline__ bool core_pair_within(int a, int q, const uint8_t* __restrict__ core, double r2) const {
    return core[a] && core[q] && d2(a, q) <= r2;
  }
};
struct CoordsF32 {
  float4* p;  // .w: 1.0f once the point is known to be a core point (k_core_*), else 0
  __device__ __forceinline__ void get(int q, double& a, double& b, double& c) const {
    const float4 v = p[q];
    a = double(v.x);
    b = double(v.y);
    c = double(v.z);
  }
  __device__ __forceinline__ double d2(int q, double px, double py, double pz) const {
    const float4 v = p[q];
    return sqdist3(px, py, pz, double(v.x), double(v.y), double(v.z));
  }
  __device__ __forceinline__ double d2(int a, int q) const {
    const float4 u = p[a], v = p[q];
    return sqdist3(double(u.x), double(u.y), double(u.z), double(v.x), double(v.y), double(v.z));
  }
  // The core flag rides in the record's fourth word: the pair tests of the union phase then
  // touch one line per point (coordinates AND flag) instead of two.
  __device__ __forceinline__ void mark_core(int q, bool is_core) const {
    reinterpret_cast<float*>(p)[size_t(q) * 4 + 3] = is_core ? 1.0f : 0.0f;
  }
  __device__ __forceinline__ bool core_pair_within(int a, int q, const uint8_t* __restrict__, double r2) const {
    const float4 u = p[a], v = p[q];
    return u.w != 0.0f && v.w != 0.0f &&
           sqdist3(double(u.x), double(u.y), double(u.z), double(v.x), double(v.y), double(v.z)) <= r2;
  }
};

// ---- wave-tiled traversal -----------------------------------------------------------
// A wave owns 64 consecutive sorted points. Their stencils are covered by nine
// LINEAR cell-id intervals [c_first + o - 1, c_last + o + 1] (o = dy*nx + dz*nx*ny),
// each one contiguous run of the sorted arrays, so the candidates are staged through
// LDS 64 at a time with coalesced loads and read back as broadcasts: no per-lane
// gathers, no divergence. Lanes test a superset of their own 27 cells (about 3.6x
// more pairs on the benchmark forest) but each test is an LDS broadcast plus nine
// fp64 instructions instead of three L1/L2 gathers. Waves whose intervals hold more
// than kTileMax candidates (sparse layers above dense ones) take the per-lane path.

static constexpr int kTileMax = 16384;

struct Tile {
  int qb[9], qe[9];
  int total;
};

__device__ __forceinline__ Tile wave_tile(int p0, int n, Stencil st, int ncell, const CellDir& dir,
                                          const int32_t* __restrict__ cell_of) {
  Tile t;
  const int plast = p0 + 63 < n ? p0 + 63 : n - 1;
  const int c_first = __builtin_amdgcn_readfirstlane(cell_of[p0]);
  const int c_last = __builtin_amdgcn_readfirstlane(cell_of[plast]);
  // the nine intervals, sorted by lower end (they already are unless the grid has
  // fewer than three rows), then clipped against what the earlier ones cover: a wave
  // that spans more than a grid row makes neighbouring intervals overlap
  int lo[9], hi[9];
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    const int o = (w % 3 - 1) * st.nx + (w / 3 - 1) * st.nxy;
    const int a = c_first + o - 1, b = c_last + o + 1;
    lo[w] = a < 0 ? 0 : a;
    hi[w] = b > ncell - 1 ? ncell - 1 : b;
  }
  // (a stable insertion sort as compare-and-swap steps at fixed positions: everything stays in SGPRs)
#pragma unroll
  for (int i = 1; i < 9; ++i)
#pragma unroll
    for (int k = i; k > 0; --k) {
      const bool sw = lo[k - 1] > lo[k];
      const int l0 = lo[k - 1], h0 = hi[k - 1];
      lo[k - 1] = sw ? lo[k] : l0;
      hi[k - 1] = sw ? hi[k] : h0;
      lo[k] = sw ? l0 : lo[k];
      hi[k] = sw ? h0 : hi[k];
    }
  // the eighteen bounds are wave-uniform: their words are asked for together, then their slots
  // (an interval that the earlier ones cover reads entry 0 twice: an empty run)
  int cells[18], q[18];
  int prev_hi = -1;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int a = lo[r] <= prev_hi ? prev_hi + 1 : lo[r];
    cells[2 * r] = cells[2 * r + 1] = 0;
    if (a <= hi[r]) {
      cells[2 * r] = a;
      cells[2 * r + 1] = hi[r] + 1;
      prev_hi = hi[r];
    }
  }
  dir.begins(cells, q);
  t.total = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    t.qb[r] = __builtin_amdgcn_readfirstlane(q[2 * r]);
    t.qe[r] = __builtin_amdgcn_readfirstlane(q[2 * r + 1]);
    t.total += t.qe[r] - t.qb[r];
  }
  return t;
}

// Calls fn(CoordsF32{...}) or fn(CoordsF64{...}) for the storage form the grid holds.
template <class F>
inline void on_coords(const DevGrid& g, F&& fn) {
  if (g.p4)
    fn(CoordsF32{g.p4});
  else
    fn(CoordsF64{g.sx, g.sy, g.sz});
}

// ---- where a binning kernel writes a sorted point ----------------------------------------------
// The output arrays of a grid as the kernel that fills them sees them: position f of the sorted order
// gets the point's original index, its cell, its sub-cell (octant binning only) and its coordinates,
// in whichever form the grid keeps (p4, or sx / sy / sz). A kernel builds the store in its first line
// from its own `__restrict__` parameters (see the note at CellDir); arrays it does not write are null
// there, as a literal, so that their stores fold away. (The stores keep the order k_bk_sort had them in, cell_of
// and sub_of first: with `order` first that kernel spilled under its cap of 80 VGPRs,
// profiles/grid_sort_resource_usage.txt.)
struct SortedStore {
  int32_t* order;
  int32_t* cell_of;  // null: the cells are written already
  int32_t* sub_of;   // null: a grid without sub-cells
  float4* p4;        // non-null: fp32 records instead of sx / sy / sz
  double *sx, *sy, *sz;
  __device__ __forceinline__ void put(int f, int idx, int cell, double x, double y, double z, int sub = 0) const {
    if (cell_of) cell_of[f] = cell;
    if (sub_of) sub_of[f] = sub;
    order[f] = idx;
    if (p4) {  // exact: fp32 records only for fp32-representable clouds
      p4[f] = make_float4(float(x), float(y), float(z), 0.f);
    } else {
      sx[f] = x;
      sy[f] = y;
      sz[f] = z;
    }
  }
  // from an fp32 record: the grid that is sorted from them keeps fp32 records too
  __device__ __forceinline__ void put(int f, int idx, int cell, float x, float y, float z, int sub = 0) const {
    if (cell_of) cell_of[f] = cell;
    if (sub_of) sub_of[f] = sub;
    order[f] = idx;
    p4[f] = make_float4(x, y, z, 0.f);
  }
};

// Octant sub-cells: the points of every cell ordered by the octant (half cell per axis) they fall
// in. A sub-cell is identified by begin(cell) * 8 + octant (first sorted position of its cell, so
// ids are unique and need no compaction); its points are the run [rec[id].x, rec[id].x + rec[id].y).
// The count is zero for empty octants of an occupied cell; entries of unoccupied ids are never
// written and must not be read.
struct SubCells {
  int32_t* sub_of;   // [n] sub-cell id of each sorted position
  int4* rec;         // [8 n] (begin, count, -1, 0) in one 16-byte record; .z and .w are the caller's
                     // (DBSCAN: .z the sub-cell's representative, .w of a cell's first record the cell's tree)
  // four ints the bounding box's fold left zeroed, for the caller's counters (spares DBSCAN two
  // memset launches per step)
  // (+ kZeroedExtra more zeroed ints behind the four: DBSCAN's segmented list counters)
  int32_t* zeroed4 = nullptr;
};
static constexpr int kZeroedExtra = 64;

// The eight sub-cell records of the cell whose run begins at sorted position b, from its octant counts.
// (count_of(o): each count is fetched where its record is written, not all eight ahead of the stores)
template <class CountOf>
__device__ __forceinline__ void write_sub_records_of(int4* __restrict__ rec, int b, CountOf&& count_of) {
  int run = b;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int cnt = count_of(o);
    rec[size_t(b) * 8 + o] = make_int4(run, cnt, -1, 0);
    run += cnt;
  }
}
__device__ __forceinline__ void write_sub_records(int4* __restrict__ rec, int b, const int (&cnt)[8]) {
  write_sub_records_of(rec, b, [&](int o) { return cnt[o]; });
}
// the same from eight 8-bit counts packed in a u64
__device__ __forceinline__ void write_sub_records(int4* __restrict__ rec, int b, unsigned long long packed) {
  write_sub_records_of(rec, b, [&](int o) { return int((packed >> (8 * o)) & 255ull); });
}

// The grid AND its octant sub-cells in one go (what DBSCAN bins with). The two-level sort (grid.hip:
// k_bk_hist, k_bk_scatter, k_bk_sort) writes every output array once, with no scattered global atomic;
// PYQSM_DBSCAN_BIN=atomic and grids beyond 2^27 cells take one returning atomic per point (its arrival
// rank in the cell), one scatter of (index, cell, octant) and one pass that orders every cell's run by
// octant from the run's own octant bytes.
// Extents that would need more than `max_cells` cells of edge `min_cell` are first COMPRESSED
// per axis: runs of empty slabs collapse to one empty slab, which keeps exactly the adjacencies
// the 27-cell stencil and the sub-cell offsets use (two points in neighbouring slabs stay in
// neighbouring slabs, all others end up at least one empty slab apart). Only if the compressed
// grid is still too large is the edge doubled (g->cell > min_cell tells the caller).
// DBSCAN builds it in two steps, declared below: plan_grid_device (bounding box and plan), then
// bin_octants_planned (the plan read on the device) or bin_octants_host (planned on the host).

// ---- DBSCAN's grid plan on the device --------------------------------------------------------
// The grid DBSCAN bins with, as the kernels of its step read it (once per wave, scalar loads). The
// bounding box's fold kernel writes it from the box with the host's own arithmetic; the host writes
// it when it plans (axis-compressed or doubled grids, fp64 records, bits = 13, the atomic binning).
// ok == 0: every kernel that reads the plan leaves at once and writes nothing.
struct GridPlan {
  double mn[3], mx[3];  // the bounding box (mn is the grid's origin)
  double inv_cell;
  int nx, ny, nz;  // including the border cells
  int rx, ry, rz;  // interior slabs before axis compression (nx - 2 ... when there is none)
  int ncell;       // nx * ny * nz
  int nbk, bits;   // buckets of 2^bits cells of the two-level sort
  int all_f32;     // every coordinate is exactly representable in fp32
  int ok;
  unsigned seq;    // the call's sequence number (the host's read-back slot: stored last)
};
__device__ __forceinline__ Stencil plan_stencil(const GridPlan* p) { return Stencil{p->nx, p->nx * p->ny}; }
// (PlanHint, the launch shapes a device-planned call is enqueued with, lives in common.hpp: the
// context keeps the last one.)

// k_bbox, which also clears zero_n ints of zero_buf, + the fold, which writes the plan of a grid of edge
// `cell` (at most `max_cells` cells) into d_plan and into h_plan (host-mapped, coherent: no copy, no
// event; h_plan->seq = seq once the rest of it is visible to the host). Does not synchronise.
// With `speculated` (there is a hint, and bin_octants_planned follows at once) there is no fold launch: the
// binning's first kernel folds k_bbox's records, uses the plan and stores it to both places; *speculated is
// what it needs for that.
struct PlanRecords {
  const unsigned long long* part;  // k_bbox's records
  int blocks;
  int64_t max_cells;
  GridPlan* h_plan;
  unsigned seq;
};
int plan_grid_device(Ctx* c, const double* xyz, int64_t n, double cell, int64_t max_cells, const PlanHint& hint,
                     GridPlan* d_plan, GridPlan* h_plan, unsigned seq, int32_t* zero_buf, int zero_n,
                     PlanRecords* speculated = nullptr);
// Zeroed ints plan_grid_device (k_bbox) must clear for the binning below (the bucket totals, reservation
// cursors and the big-cell counter) plus kZeroedExtra + 4 for the caller.
int octant_zeroed_ints();
// The octant binning enqueued with the hint's shapes. Its first kernel plans from `rec` and writes d_plan
// (and the host's slot); every later kernel reads the grid from d_plan.
int bin_octants_planned(Ctx* c, const double* xyz, int64_t n, double cell, const PlanHint& hint,
                        const PlanRecords& rec, GridPlan* d_plan, int32_t* zeroed, DevGrid* g, SubCells* sub);
// The octant binning planned on the host from the box and fp32 flag of `box` (read back from
// plan_grid_device; finite-checked here: PYQSM_EINVAL). Writes the exact plan to *h_exact, uploads
// it through h_up (page-locked) to d_plan, and *hint_out = the hint it makes (valid = 0: the grid is
// not of the device-plannable kind).
int bin_octants_host(Ctx* c, const double* xyz, int64_t n, double min_cell, int64_t max_cells, const GridPlan& box,
                     int32_t* zeroed, GridPlan* h_up, GridPlan* d_plan, DevGrid* g, SubCells* sub,
                     PlanHint* hint_out);

// The device begin(c) of g's ranked directory for c = 0 .. ncell into begin_out (device, [ncell + 1]):
// the read-out the tests compare with a dense count (ncell: the plan's, read on the host by the caller).
void read_directory(Ctx* c, const DevGrid& g, int64_t ncell, int32_t* begin_out);

// A grid with cells `factor` times larger over the same points, derived from `fine`
// by block sums and a deterministic scatter (no atomics, no second pass over xyz).
int coarsen_grid(Ctx* c, const DevGrid& fine, int64_t n, int factor, DevGrid* coarse);

// ---- what the fixed-radius kernels share (radius, adjacency, grow, normals, features) -----------
// The grid a ball query walks: `d_src` binned into cells of edge `radius` (times 1 + 2^-20, so that an
// inclusive bound stays inside the 27 cells), at most 2^28 cells, over the cloud without its sparse
// tails (cloud_bbox -> robust_box -> build_grid; the tails may hold one point in 256, no fewer than
// 256 and no more than 8192); fp32 records when every coordinate allows. Points the box gave up sit in its outermost
// cells, and queries find them through clamped_cell. cloud_box (optional): min xyz, max xyz of the
// whole cloud, tails included.
int ball_grid(Ctx* c, const double* d_src, int64_t n, double radius, DevGrid* g, double* cloud_box = nullptr);
// ball_grid, and inside a cell the points in ascending original index (not in the arrival order
// build_grid leaves), so the order in which a query walks its candidates, and with it its choice among
// ties at the k-th distance, is the same for every build over the same cloud.
int radius_grid(Ctx* c, const double* d_src, int64_t n, double radius, DevGrid* g);
// *perm = the m query points (f64 [m,3], device) in the order of the grid's cells, or nullptr for
// fewer than 1024 queries (or PYQSM_RADIUS_SORT=0): serve them in the caller's order.
int query_order(Ctx* c, const double* d_qry, int64_t m, const GridParams& rg, int64_t ncell, int32_t** perm);

// Number of occupied cells (reads back one int; synchronises).
int count_occupied(Ctx* c, const DevGrid& g, int64_t* occupied);

}  // namespace pyqsm
