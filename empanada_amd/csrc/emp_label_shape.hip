// Shape descriptors of the objects of a label volume (include/emp_hip.h, E11): per label the voxel count, first and
// second index sums, the intercept ends along the 13 lattice directions and the lattice corners and edges it owns.
// What users of the reference get on a CPU afterwards, object by object, from MorphoLibJ or regionprops; the
// definition is the header's.
//
// Every column is a sum over the voxels of a function of the voxel's mask M of same-label neighbours (E8's numbering,
// emp_common.h): cross_k = 2 - bit (13 + k) - bit (12 - k), and a corner or edge of the voxel's cube is the voxel's own
// iff no same-label voxel around it comes earlier in (z, y, x) order: (M & PRE) == 0 for a constant mask PRE, built
// here by constexpr functions from the numbering, as LT_ADJ26 is.
//
// Tile: 8 x 8 x 64 voxels and 256 threads, as emp_label_thin.hip; a block walks tiles and leaves one whose own voxels
// are all background after reading them.  Otherwise it stages the tile with its one-voxel ring in LDS (10 x 10 x 66
// words), and every thread visits 16 voxels of one x, summing in registers while the label stays the same -- index
// products relative to the tile's origin, so that a tile's sums fit 32 bits, and the 15 counts as 16-bit halves.  What
// a thread holds at the end is folded over the lanes that are adjacent in x and hold the same label (a segmented
// scan), and the last lane of each such group adds to the tile's table in LDS: LS_SLOTS labels, open addressing, LDS
// integer atomics.  The table is then flushed, one 64-bit atomic per (label, column) that is not zero, after shifting
// the local moments to global indices exactly.  A label that finds the table full sends its sums straight to its row:
// correct, slow, counted.  Integer adds only, so neither the arrival order nor which labels overflowed shows.
#include "emp_common.h"

#define LS_PZ (EMP_TILE_Z + 2)
#define LS_PY (EMP_TILE_Y + 2)
#define LS_PX (EMP_TILE_X + 2)
#define LS_CELLS (LS_PZ * LS_PY * LS_PX)
#define LS_VOX (EMP_TILE_Z * EMP_TILE_Y * EMP_TILE_X)
#define LS_THREADS 256
#define LS_COLS 26
#define LS_SUMS (LS_COLS - 1)   // the columns after the label
#define LS_MOM 10               // of which moments: n, z, y, x, zz, yy, xx, zy, zx, yx
#define LS_WORDS (LS_MOM + 8)   // a thread's sums: the moments and the 15 counts, two to a word
#define LS_SLOTS 16
#define LS_MAX_INDEX (1LL << 20)

typedef unsigned long long ls_u64;

// ------------------------------------------------------------------------------------------ ownership masks
// The voxels around corner c = (cz, cy, cx) of the cube of the voxel at offset 0 sit at the offsets o with o_a in
// {c_a - 1, c_a}; those before the voxel itself in (z, y, x) order are the positions below the centre, bits 0 .. 12.
static constexpr bool ls_beside(int o, int c) { return o == 0 || o == (c ? 1 : -1); }
static constexpr uint32_t ls_pre_corner(int c)
{
    uint32_t m = 0;
    for (int n = 0; n < 13; ++n)
        if (ls_beside(lt_dz(n), (c >> 2) & 1) && ls_beside(lt_dy(n), (c >> 1) & 1) && ls_beside(lt_dx(n), c & 1))
            m |= 1u << n;
    return m;
}
// edge e: along axis e / 4 (0 = z, 1 = y, 2 = x), at corner (e >> 1 & 1, e & 1) of the two other axes in (z, y, x) order
static constexpr uint32_t ls_pre_edge(int e)
{
    const int axis = e / 4, c0 = (e >> 1) & 1, c1 = e & 1;
    uint32_t m = 0;
    for (int n = 0; n < 13; ++n) {
        const int o[3] = {lt_dz(n), lt_dy(n), lt_dx(n)};
        const int b0 = axis == 0 ? 1 : 0, b1 = axis == 2 ? 1 : 2;
        if (o[axis] == 0 && ls_beside(o[b0], c0) && ls_beside(o[b1], c1)) m |= 1u << n;
    }
    return m;
}
static constexpr int ls_pre_total(bool edges)
{
    int t = 0;
    for (int i = 0; i < (edges ? 12 : 8); ++i) t += __builtin_popcount(edges ? ls_pre_edge(i) : ls_pre_corner(i));
    return t;
}
// every pair of voxels around a corner (8 * 7 / 2 per corner position) or an edge (4 * 3 / 2) is ordered one way
static_assert(__builtin_popcount(ls_pre_corner(0)) == 7 && ls_pre_corner(7) == 0 && ls_pre_total(false) == 28,
              "corner ownership");
static_assert(__builtin_popcount(ls_pre_edge(0)) == 3 && ls_pre_edge(3) == 0 && ls_pre_edge(7) == 0 &&
                  ls_pre_edge(11) == 0 && ls_pre_total(true) == 18,
              "edge ownership");
// bit 13 + k and bit 12 - k of M are the two ends of direction k
static_assert(lt_dz(13) == 0 && lt_dy(13) == 0 && lt_dx(13) == 1 && lt_dz(21) == 1 && lt_dy(21) == 0 && lt_dx(21) == 0 &&
                  lt_dz(4) == -1 && lt_dy(4) == 0 && lt_dx(4) == 0 && lt_dx(12) == -1,
              "direction codes");

// ------------------------------------------------------------------------------------------ a thread's sums
// column j + 1 of the table out of the packed words
__device__ __forceinline__ uint32_t ls_unpack(const uint32_t *a, int j)
{
    return j < LS_MOM ? a[j] : (a[LS_MOM + ((j - LS_MOM) >> 1)] >> (16 * ((j - LS_MOM) & 1))) & 0xffffu;
}

// Column j + 1 in global indices from sums taken relative to (z0, y0, x0): m holds the ten local moments and `own` the
// local value of column j + 1.  sum (z0 + z')^2 = n z0^2 + 2 z0 sum z' + sum z'^2, and likewise for the mixed products.
__device__ __forceinline__ ls_u64 ls_shift(int j, const uint32_t *m, uint32_t own, ls_u64 z0, ls_u64 y0, ls_u64 x0)
{
    const ls_u64 n = m[0], sz = m[1], sy = m[2], sx = m[3];
    switch (j) {
    case 1: return n * z0 + sz;
    case 2: return n * y0 + sy;
    case 3: return n * x0 + sx;
    case 4: return n * z0 * z0 + 2ull * z0 * sz + m[4];
    case 5: return n * y0 * y0 + 2ull * y0 * sy + m[5];
    case 6: return n * x0 * x0 + 2ull * x0 * sx + m[6];
    case 7: return n * z0 * y0 + z0 * sy + y0 * sz + m[7];
    case 8: return n * z0 * x0 + z0 * sx + x0 * sz + m[8];
    case 9: return n * y0 * x0 + y0 * sx + x0 * sy + m[9];
    default: return own;
    }
}

// the row of `label` among the block's sorted labels, -1 if it is not there
__device__ __forceinline__ int64_t ls_row(const uint32_t *__restrict__ labels, int64_t n, uint32_t label)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (labels[mid] < label) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && labels[lo] == label) ? lo : -1;
}

// the slot of `label` in the tile's table, claimed if it has none yet; -1: the table is full
__device__ __forceinline__ int ls_slot(uint32_t *s_key, uint32_t label)
{
    const uint32_t h = (label * 2654435761u) >> 28;
#pragma unroll 1
    for (int i = 0; i < LS_SLOTS; ++i) {
        const int s = (int)((h + i) & (LS_SLOTS - 1));
        uint32_t k = __hip_atomic_load(s_key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0u) {
            k = atomicCAS(s_key + s, 0u, label);
            if (k == 0u) return s;
        }
        if (k == label) return s;
    }
    return -1;
}

struct LsOut {
    const uint32_t *labels;
    int64_t n_labels;
    ls_u64 *table, *counters;
};

// what a thread (or the last lane of a group) holds of `label` goes to the tile's table, or to the label's row
__device__ __forceinline__ void ls_commit(uint32_t label, const uint32_t *a, uint32_t *s_key, uint32_t (*s_sum)[LS_SUMS],
                                          unsigned *s_spilled, const LsOut &o, ls_u64 z0, ls_u64 y0, ls_u64 x0)
{
    const int slot = ls_slot(s_key, label);
    if (slot >= 0) {
#pragma unroll
        for (int j = 0; j < LS_SUMS; ++j) {
            const uint32_t v = ls_unpack(a, j);
            if (v) atomicAdd(&s_sum[slot][j], v);
        }
        return;
    }
    atomicAdd(s_spilled, a[0]);
    const int64_t row = ls_row(o.labels, o.n_labels, label);
    if (row < 0) return;
#pragma unroll
    for (int j = 0; j < LS_SUMS; ++j) {
        const ls_u64 v = ls_shift(j, a, ls_unpack(a, j), z0, y0, x0);
        if (v) atomicAdd(o.table + row * LS_COLS + 1 + j, v);
    }
}

// ------------------------------------------------------------------------------------------ the pass
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void ls_tile_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                             EmpTiles tiles, const T *__restrict__ below,
                                                             const T *__restrict__ above, int64_t z_base, LsOut o)
{
    __shared__ uint32_t s_obj[LS_CELLS];
    __shared__ uint32_t s_key[LS_SLOTS];
    __shared__ uint32_t s_sum[LS_SLOTS][LS_SUMS];
    __shared__ int64_t s_row[LS_SLOTS];
    __shared__ unsigned s_spilled;
    const int t = threadIdx.x, lane = t & 63;
    for (int64_t tile = blockIdx.x; tile < tiles.n; tile += gridDim.x) {
        const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
        const int64_t z0 = tz * EMP_TILE_Z, y0 = ty * EMP_TILE_Y, x0 = tx * EMP_TILE_X;
        // 1. the tile's own voxels; a tile of background alone ends here
        if (t < LS_SLOTS) s_key[t] = 0u;
        for (int i = t; i < LS_SLOTS * LS_SUMS; i += LS_THREADS) s_sum[i / LS_SUMS][i % LS_SUMS] = 0u;
        if (t == 0) s_spilled = 0u;
        int any = 0;
        for (int i = t; i < LS_VOX; i += LS_THREADS) {
            const int lx = i & (EMP_TILE_X - 1), ly = (i / EMP_TILE_X) & (EMP_TILE_Y - 1), lz = i / (EMP_TILE_X * EMP_TILE_Y);
            const int64_t z = z0 + lz, y = y0 + ly, x = x0 + lx;
            // a cell of the tile past the block's last slice is no voxel of the block, but holds the slice above it
            const bool own = z < D && y < H && x < W;
            const uint32_t v = own ? (uint32_t)lab[(z * H + y) * W + x] : lt_label_at<T>(lab, below, above, D, H, W, z, y, x);
            s_obj[((lz + 1) * LS_PY + ly + 1) * LS_PX + lx + 1] = v;
            any |= own && v != 0u;
        }
        if (!__syncthreads_or(any)) continue;
        // 2. its ring
        for (int c = t; c < LS_CELLS; c += LS_THREADS) {
            const int lx = c % LS_PX, ly = (c / LS_PX) % LS_PY, lz = c / (LS_PX * LS_PY);
            if (lz >= 1 && lz <= EMP_TILE_Z && ly >= 1 && ly <= EMP_TILE_Y && lx >= 1 && lx <= EMP_TILE_X) continue;
            s_obj[c] = lt_label_at<T>(lab, below, above, D, H, W, z0 - 1 + lz, y0 - 1 + ly, x0 - 1 + lx);
        }
        __syncthreads();
        // 3. 16 voxels of one x per thread: rows (z', y') = wave, wave + 4, ...
        const ls_u64 gz = (ls_u64)(z_base + z0), gy = (ls_u64)y0, gx = (ls_u64)x0;
        uint32_t a[LS_WORDS];
#pragma unroll
        for (int w = 0; w < LS_WORDS; ++w) a[w] = 0u;
        uint32_t cur = 0u;
        for (int i = t; i < LS_VOX; i += LS_THREADS) {
            const uint32_t lx = (uint32_t)lane, ly = (uint32_t)(i / EMP_TILE_X) & (EMP_TILE_Y - 1),
                           lz = (uint32_t)i / (EMP_TILE_X * EMP_TILE_Y);
            const int c = (int)(((lz + 1) * LS_PY + ly + 1) * LS_PX + lx + 1);
            const uint32_t l = s_obj[c];
            if (l == 0u || z0 + (int64_t)lz >= D) continue;
            if (l != cur) {
                if (cur != 0u) ls_commit(cur, a, s_key, s_sum, &s_spilled, o, gz, gy, gx);
#pragma unroll
                for (int w = 0; w < LS_WORDS; ++w) a[w] = 0u;
                cur = l;
            }
            uint32_t M = 0u;
#pragma unroll
            for (int n = 0; n < 26; ++n)
                M |= (s_obj[c + (lt_dz(n) * LS_PY + lt_dy(n)) * LS_PX + lt_dx(n)] == l ? 1u : 0u) << n;
            a[0] += 1u;
            a[1] += lz;
            a[2] += ly;
            a[3] += lx;
            a[4] += lz * lz;
            a[5] += ly * ly;
            a[6] += lx * lx;
            a[7] += lz * ly;
            a[8] += lz * lx;
            a[9] += ly * lx;
            // bit k of up / dn: the neighbour at + d_k / - d_k does not carry the label
            const uint32_t up = ~(M >> 13) & 0x1fffu, dn = ~(__brev(M) >> 19) & 0x1fffu;
            uint32_t corners = 0u, edges = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) corners += (M & ls_pre_corner(k)) == 0u ? 1u : 0u;
#pragma unroll
            for (int k = 0; k < 12; ++k) edges += (M & ls_pre_edge(k)) == 0u ? 1u : 0u;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                a[LS_MOM + k] += ((up >> (2 * k)) & 1u) + ((dn >> (2 * k)) & 1u) +
                                 ((((up >> (2 * k + 1)) & 1u) + ((dn >> (2 * k + 1)) & 1u)) << 16);
            a[LS_MOM + 6] += ((up >> 12) & 1u) + ((dn >> 12) & 1u) + (corners << 16);
            a[LS_MOM + 7] += edges;
        }
        // 4. lanes that are neighbours in x and hold the same label fold into the last of them: at most 16 voxels per
        //    lane, so a 16-bit half holds at most 64 * 16 * 12
        const uint32_t prev = __shfl_up(cur, 1);
        const ls_u64 heads = __ballot(lane == 0 || prev != cur);
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));    // the group's first lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
            for (int w = 0; w < LS_WORDS; ++w) {
                const uint32_t b = __shfl_up(a[w], d);
                if (lane - d >= start) a[w] += b;
            }
        }
        if (cur != 0u && (lane == 63 || ((heads >> (lane + 1)) & 1ull)))
            ls_commit(cur, a, s_key, s_sum, &s_spilled, o, gz, gy, gx);
        __syncthreads();
        // 5. the tile's table goes to the rows of its labels
        if (t < LS_SLOTS) s_row[t] = s_key[t] ? ls_row(o.labels, o.n_labels, s_key[t]) : -1;
        __syncthreads();
        for (int i = t; i < LS_SLOTS * LS_SUMS; i += LS_THREADS) {
            const int slot = i / LS_SUMS, j = i % LS_SUMS;
            const int64_t row = s_row[slot];
            if (row < 0) continue;
            uint32_t m[LS_MOM];
#pragma unroll
            for (int w = 0; w < LS_MOM; ++w) m[w] = s_sum[slot][w];
            const ls_u64 v = ls_shift(j, m, s_sum[slot][j], gz, gy, gx);
            if (v) atomicAdd(o.table + row * LS_COLS + 1 + j, v);
        }
        if (t == 0) {
            atomicAdd(o.counters, 1ull);
            if (s_spilled) atomicAdd(o.counters + 1, (ls_u64)s_spilled);
        }
        __syncthreads();                      // the next tile clears the table
    }
}

// label in column 0, zero in every sum; the two counters
__global__ void ls_init_kernel(const uint32_t *__restrict__ labels, int64_t n_labels, int64_t *__restrict__ table,
                               int64_t *__restrict__ counters)
{
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 < 2) counters[i0] = 0;
    for (int64_t i = i0; i < n_labels * LS_COLS; i += (int64_t)gridDim.x * blockDim.x)
        table[i] = (i % LS_COLS) == 0 ? (int64_t)labels[i / LS_COLS] : 0LL;
}

#define LS_REQUIRE_SHAPE(what)                                                                                         \
    do {                                                                                                               \
        EMP_REQUIRE_VOLUME(what);                                                                                      \
        EMP_REQUIRE(emp_tiles_shape_ok(D, H, W),                                                                       \
                    what ": %lld x %lld x %lld voxels are more than 2^31 - 1; cut the slab into z-blocks",             \
                    (long long)D, (long long)H, (long long)W);                                                         \
        EMP_REQUIRE(D == 0 || lab, what ": null pointer");                                                             \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0, what ": misaligned labels");            \
    } while (0)

extern "C" int emp_label_shape(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                               const void *above, int64_t z_base, const uint32_t *labels, int64_t n_labels,
                               int64_t *out_table, int64_t *counters, void *stream)
{
    LS_REQUIRE_SHAPE("label_shape");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(below) % (uintptr_t)item) == 0 &&
                    (reinterpret_cast<uintptr_t>(above) % (uintptr_t)item) == 0,
                "label_shape: misaligned neighbour slice");
    EMP_REQUIRE(z_base >= 0 && z_base <= LS_MAX_INDEX && z_base + D <= LS_MAX_INDEX && H <= LS_MAX_INDEX &&
                    W <= LS_MAX_INDEX,
                "label_shape: z_base + D = %lld + %lld, H = %lld, W = %lld: every index must stay below 2^20",
                (long long)z_base, (long long)D, (long long)H, (long long)W);
    EMP_REQUIRE(n_labels >= 0 && n_labels <= D * H * W, "label_shape: %lld labels in %lld voxels", (long long)n_labels,
                (long long)(D * H * W));
    EMP_REQUIRE(counters && (n_labels == 0 || (labels && out_table)), "label_shape: null pointer");
    hipStream_t st = emp_stream(stream);
    EMP_LAUNCH(ls_init_kernel, emp_grid(n_labels * LS_COLS, 256, 4096), 256, st, labels, n_labels, out_table, counters);
    if (D == 0 || n_labels == 0) return EMP_OK;
    const EmpTiles T = emp_tiles(D, H, W);
    LsOut o;
    o.labels = labels;
    o.n_labels = n_labels;
    o.table = reinterpret_cast<ls_u64 *>(out_table);
    o.counters = reinterpret_cast<ls_u64 *>(counters);
    const int grid = emp_grid(T.n, 1, 8192);
    if (item == 4)
        EMP_LAUNCH((ls_tile_kernel<uint32_t>), grid, LS_THREADS, st, reinterpret_cast<const uint32_t *>(lab), D, H, W, T,
                   reinterpret_cast<const uint32_t *>(below), reinterpret_cast<const uint32_t *>(above), z_base, o);
    else
        EMP_LAUNCH((ls_tile_kernel<uint8_t>), grid, LS_THREADS, st, reinterpret_cast<const uint8_t *>(lab), D, H, W, T,
                   reinterpret_cast<const uint8_t *>(below), reinterpret_cast<const uint8_t *>(above), z_base, o);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ the labels of a block
// One record per run of E2's step 1 (the run extraction of emp_measure.hip without the neighbour rows), sorted by
// label; the first of every label is kept.
struct LsWork {
    int32_t *row, *xs, *xe;
    uint32_t *val;
    uint64_t *keys, *keys_out;
    int32_t *idx, *idx_out, *head, *pos, *scantmp;
    char *cub;
    int64_t cub_bytes, total;
};
static LsWork ls_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    LsWork L;
    L.row = c.take<int32_t>(n);
    L.xs = c.take<int32_t>(n);
    L.xe = c.take<int32_t>(n);
    L.val = c.take<uint32_t>(n);
    L.keys = c.take<uint64_t>(n);
    L.keys_out = c.take<uint64_t>(n);
    L.idx = c.take<int32_t>(n);
    L.idx_out = c.take<int32_t>(n);
    // the run records are dead once the keys are made
    L.head = L.row;
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.cub_bytes = emp_sort_work_bytes(n);
    L.cub = c.take<char>(L.cub_bytes);
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_label_shape_work_bytes(int64_t n_runs) { return n_runs < 0 ? -1 : ls_carve(nullptr, n_runs).total; }

__global__ void ls_keys_kernel(const uint32_t *__restrict__ val, int64_t n, uint64_t *__restrict__ keys,
                               int32_t *__restrict__ idx)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (uint64_t)val[i];
        idx[i] = (int32_t)i;
    }
}

__global__ void ls_labels_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ head,
                                 const int32_t *__restrict__ pos, int64_t n, uint32_t *__restrict__ labels)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (head[i]) labels[pos[i]] = (uint32_t)keys[i];
}

extern "C" int emp_label_shape_labels(const void *lab, int item, int64_t D, int64_t H, int64_t W,
                                      const int32_t *row_offsets, int64_t n_runs, void *work, int64_t work_bytes,
                                      uint32_t *labels, int32_t *n_out, void *stream)
{
    LS_REQUIRE_SHAPE("label_shape_labels");
    EMP_REQUIRE(row_offsets && n_out, "label_shape_labels: null pointer");
    EMP_REQUIRE(n_runs >= 0 && n_runs <= D * H * W,
                "label_shape_labels: n_runs = %lld is not the run total of %lld voxels", (long long)n_runs,
                (long long)(D * H * W));
    hipStream_t st = emp_stream(stream);
    if (n_runs == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_out, (int64_t)1);
        return EMP_OK;
    }
    EMP_REQUIRE(work && labels, "label_shape_labels: null pointer");
    LsWork L = ls_carve(work, n_runs);
    EMP_REQUIRE(work_bytes >= L.total, "label_shape_labels: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    int rc = emp_label_rows_extract(lab, item, D, H, W, row_offsets, n_runs, L.row, L.xs, L.xe, L.val, stream);
    if (rc != EMP_OK) return rc;
    const int grid = emp_grid(n_runs, 256, 4096);
    EMP_LAUNCH(ls_keys_kernel, grid, 256, st, L.val, n_runs, L.keys, L.idx);
    rc = emp_sort_u64_i32(L.keys, L.keys_out, L.idx, L.idx_out, n_runs, 0, 32, L.cub, L.cub_bytes, stream);
    if (rc != EMP_OK) return rc;
    return emp_compact(
        L.head, n_runs, L.pos, L.scantmp, n_out, stream, "label_shape_labels: count copy",
        [&]() -> int {
            EMP_LAUNCH(emp_heads_kernel<0>, grid, 256, st, L.keys_out, n_runs, L.head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(ls_labels_kernel, grid, 256, st, L.keys_out, L.head, L.pos, n_runs, labels);
            return EMP_OK;
        });
}
