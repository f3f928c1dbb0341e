// Background cavities of a label volume (include/emp_hip.h, E4): one row per 6-connected component of the ZERO voxels
// with its voxel count, first voxel, box and the smallest and largest label on its wall.  What users of the reference
// do on a CPU afterwards with scipy.ndimage.binary_fill_holes, object by object; the definition is the header's.
//
// Count -> scan -> extract over the runs of zero voxels per row, then emp_components.hip's union-find over the runs
// (all of value 0, connectivity 6), its numbering of the roots and its workspace layout, so that its paint kernel
// writes the fill.  Two things differ from E3.  The statistics are reduced over the wave before any atomic: the
// outside background is ONE component that holds most runs of the volume, and one atomic per run on its row would
// serialise.  And the wall labels are surveyed last, only for the runs of components whose box keeps clear of the
// block's x and y borders: the others are open whatever their wall is, so the survey costs the voxels of candidate
// cavities, not of the volume.
#include "emp_common.h"

#define HL_COLS 10
#define HL_NO_LABEL 0x100000000LL

// bit j: voxel x + j lies inside the row and is zero.  One aligned load (16 bytes of uint32, 4 of uint8) where the
// group lies inside the row on such an address, voxel by voxel otherwise: the same bits.
template <typename T>
__device__ __forceinline__ uint32_t hl_zero_mask(const T *__restrict__ src, int64_t x, int64_t W)
{
    uint32_t m = 0u;
    if (x >= 0 && x + 4 <= W && (reinterpret_cast<uintptr_t>(src + x) & (uintptr_t)(4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + x);
            m = (uint32_t)(q.x == 0u) | ((uint32_t)(q.y == 0u) << 1) | ((uint32_t)(q.z == 0u) << 2) |
                ((uint32_t)(q.w == 0u) << 3);
        } else {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(src + x);
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= (uint32_t)(((q >> (8 * j)) & 0xffu) == 0u) << j;
        }
        return m;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x + j >= 0 && x + j < W && src[x + j] == (T)0) m |= 1u << j;
    return m;
}

// One wave per row, 4 consecutive voxels per lane, the lane grid shifted so that full groups are aligned loads for any
// W and base offset (as ms_rows_kernel).  A run starts on a zero voxel whose left neighbour is not one and ends on a
// zero voxel whose right neighbour is not one; positions outside the row are not zero voxels.
template <typename T, bool EXTRACT>
__global__ __launch_bounds__(256) void hl_rows_kernel(const T *__restrict__ lab, int64_t n_rows, int64_t W,
                                                      int32_t *__restrict__ row_counts,
                                                      const int32_t *__restrict__ row_offsets, int64_t n_runs,
                                                      int32_t *__restrict__ o_row, int32_t *__restrict__ o_xs,
                                                      int32_t *__restrict__ o_xe)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long before = (1ull << lane) - 1ull;
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        const T *src = lab + row * W;
        const int shift = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & 3);
        const int32_t obase = EXTRACT ? row_offsets[row] : 0;
        int n_s = 0, n_e = 0;                                           // wave-uniform counts of starts / ends so far
        uint32_t m = hl_zero_mask<T>(src, (int64_t)lane * 4 - shift, W);
        uint32_t carry = 0u;                                            // was the voxel left of the chunk a zero voxel
        for (int64_t x0 = -shift; x0 < W; x0 += 256) {
            const int64_t x = x0 + (int64_t)lane * 4;
            const uint32_t nx = x0 + 256 < W ? hl_zero_mask<T>(src, x + 256, W) : 0u;
            if (__ballot(m != 0u) == 0ull) {                            // no zero voxel in the chunk: nothing starts or ends
                carry = 0u;
                m = nx;
                continue;
            }
            uint32_t left = (__shfl_up(m, 1) >> 3) & 1u, right = __shfl_down(m, 1) & 1u;
            const uint32_t first_next = __shfl(nx, 0) & 1u;
            if (lane == 0) left = carry;
            if (lane == 63) right = first_next;
            const uint32_t prev = ((m << 1) | left) & 0xfu, next = (m >> 1) | (right << 3);
            const uint32_t st = m & ~prev, en = m & ~next;
            int tot_s = 0, tot_e = 0, ps = 0, pe = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long bs = __ballot((st >> j) & 1u), be = __ballot((en >> j) & 1u);
                tot_s += __popcll(bs);
                tot_e += __popcll(be);
                if (EXTRACT) {
                    ps += __popcll(bs & before);
                    pe += __popcll(be & before);
                }
            }
            if (EXTRACT) {
                int64_t is = (int64_t)obase + n_s + ps, ie = (int64_t)obase + n_e + pe;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((st >> j) & 1u) {
                        if (is < n_runs) {
                            o_row[is] = (int32_t)row;
                            o_xs[is] = (int32_t)(x + j);
                        }
                        ++is;
                    }
                    if ((en >> j) & 1u) {
                        if (ie < n_runs) o_xe[ie] = (int32_t)(x + j + 1);
                        ++ie;
                    }
                }
            }
            n_s += tot_s;
            n_e += tot_e;
            carry = (__shfl(m, 63) >> 3) & 1u;
            m = nx;
        }
        if (!EXTRACT && lane == 0) row_counts[row] = n_s;
    }
}

// pos[root] numbers the roots in run order; the root's own thread starts the component's row
__global__ void hl_comp_kernel(int64_t n, int64_t W, int64_t first_base, const int32_t *__restrict__ parent,
                               const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                               const int32_t *__restrict__ row, const int32_t *__restrict__ xs,
                               int32_t *__restrict__ comp, int64_t *__restrict__ table)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = pos[parent[i]];
        comp[i] = k;
        if (flag[i]) {
            int64_t *t = table + (int64_t)k * HL_COLS;
            t[0] = 0;
            t[1] = first_base + (int64_t)row[i] * W + xs[i];
            t[2] = t[3] = t[4] = 0x7fffffffffffffffLL;
            t[5] = t[6] = t[7] = 0;
            t[8] = HL_NO_LABEL;
            t[9] = 0;
        }
    }
}

// Voxels and boxes.  A wave takes 64 * HL_SEG consecutive runs, lane l the runs l, l + 64, ...: runs are in raster
// order, so nearly all of them belong to the component the lane already holds (the outside background holds most runs
// of a volume) and are folded in registers.  A run of another component is sent to its own row at once and what is
// held stays -- a cavity's row is met by few runs, the outside's by millions, and giving up the outside's partial sum
// for every cavity run would put those sends back onto its row; only a lane that holds a single run swaps.
// What the lanes hold at the end is folded over the wave by a segmented scan (a segment = consecutive lanes of one
// component) and the last lane of every segment alone touches the table -- one add per segment, and a minimum or
// maximum only where it improves on what the row holds (a minimum only falls and a maximum only rises, so a value read
// earlier is never better than the current one).  Integer add / min / max: neither the grouping nor the order of the
// atomics shows.
#define HL_SEG 16
struct HlAcc {
    unsigned long long vox;
    int z0, y0, x0, z1, y1, x1;                              // z local to the block
    __device__ void reset()
    {
        vox = 0ull;
        z0 = y0 = x0 = 0x7fffffff;
        z1 = y1 = x1 = 0;
    }
    __device__ void flush(int64_t *__restrict__ row, int64_t z_base) const
    {
        unsigned long long *t = reinterpret_cast<unsigned long long *>(row);
        const unsigned long long Z0 = (unsigned long long)(z_base + z0), Z1 = (unsigned long long)(z_base + z1);
        atomicAdd(t + 0, vox);
        if (Z0 < t[2]) atomicMin(t + 2, Z0);
        if ((unsigned long long)y0 < t[3]) atomicMin(t + 3, (unsigned long long)y0);
        if ((unsigned long long)x0 < t[4]) atomicMin(t + 4, (unsigned long long)x0);
        if (Z1 > t[5]) atomicMax(t + 5, Z1);
        if ((unsigned long long)y1 > t[6]) atomicMax(t + 6, (unsigned long long)y1);
        if ((unsigned long long)x1 > t[7]) atomicMax(t + 7, (unsigned long long)x1);
    }
};

__global__ __launch_bounds__(256) void hl_stats_kernel(int64_t n, int64_t H, int64_t z_base,
                                                       const int32_t *__restrict__ row, const int32_t *__restrict__ xs,
                                                       const int32_t *__restrict__ xe, const int32_t *__restrict__ comp,
                                                       int64_t *__restrict__ table)
{
    const int lane = threadIdx.x & 63;
    const int64_t chunk = 64 * HL_SEG;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    // base is wave uniform, so that every lane takes part in the shuffles
    for (int64_t base = wave * chunk; base < n; base += n_waves * chunk) {
        int k = -1, held = 0;                                // the component held and how many of its runs; none yet
        HlAcc a;
        a.reset();
#pragma unroll 4
        for (int j = 0; j < HL_SEG; ++j) {
            const int64_t i = base + (int64_t)j * 64 + lane;
            if (i >= n) break;
            const int a0 = xs[i], a1 = xe[i];
            if (a1 <= a0) continue;                          // an empty slot
            const int64_t r = row[i];
            const int kk = comp[i];
            const int z = (int)(r / H), y = (int)(r - (int64_t)z * H);
            if (kk != k) {
                if (held > 1) {                              // keep what is held: this run goes to its row on its own
                    HlAcc one;
                    one.vox = (unsigned long long)(a1 - a0);
                    one.z0 = z; one.z1 = z + 1; one.y0 = y; one.y1 = y + 1; one.x0 = a0; one.x1 = a1;
                    one.flush(table + (int64_t)kk * HL_COLS, z_base);
                    continue;
                }
                if (held > 0) a.flush(table + (int64_t)k * HL_COLS, z_base);
                a.reset();
                k = kk;
                held = 0;
            }
            ++held;
            a.vox += (unsigned long long)(a1 - a0);
            a.z0 = min(a.z0, z); a.z1 = max(a.z1, z + 1);
            a.y0 = min(a.y0, y); a.y1 = max(a.y1, y + 1);
            a.x0 = min(a.x0, a0); a.x1 = max(a.x1, a1);
        }
        const int pk = __shfl_up(k, 1);
        int f = (lane == 0 || pk != k) ? 1 : 0;              // head of a segment
        const int next_head = __shfl_down(f, 1);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long bv = __shfl_up(a.vox, d);
            const int bz0 = __shfl_up(a.z0, d), by0 = __shfl_up(a.y0, d), bx0 = __shfl_up(a.x0, d);
            const int bz1 = __shfl_up(a.z1, d), by1 = __shfl_up(a.y1, d), bx1 = __shfl_up(a.x1, d);
            const int bf = __shfl_up(f, d);
            if (lane >= d && !f) {
                a.vox += bv;
                a.z0 = min(a.z0, bz0); a.y0 = min(a.y0, by0); a.x0 = min(a.x0, bx0);
                a.z1 = max(a.z1, bz1); a.y1 = max(a.y1, by1); a.x1 = max(a.x1, bx1);
                f = bf;
            }
        }
        if (k >= 0 && (lane == 63 || next_head)) a.flush(table + (int64_t)k * HL_COLS, z_base);
    }
}

// The wall labels, after the boxes are complete.  16 lanes per run; a run of a component whose box touches x = 0,
// x = W, y = 0 or y = H of the block is skipped (open whatever its wall is), so every run that is surveyed has a voxel
// before and after it and a row on either side in y.  Along z the rows of the block, `below` / `above` at its ends, or
// nothing.  Only the x range of the run itself is read in the four rows: an edge or corner contact is no wall.
template <typename T>
__global__ __launch_bounds__(256) void hl_survey_kernel(int64_t n, int64_t D, int64_t H, int64_t W,
                                                        const T *__restrict__ lab, const T *__restrict__ below,
                                                        const T *__restrict__ above, const int32_t *__restrict__ row,
                                                        const int32_t *__restrict__ xs, const int32_t *__restrict__ xe,
                                                        const int32_t *__restrict__ comp, int64_t *__restrict__ table)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) >> 4;
    const int64_t n_rows = D * H;
    for (int64_t i = group; i < n; i += n_groups) {
        const int64_t r = row[i], a0 = xs[i], a1 = xe[i];
        if (r < 0 || r >= n_rows || a0 < 1 || a1 >= W || a1 <= a0) continue;
        int64_t *t = table + (int64_t)comp[i] * HL_COLS;
        if (t[3] < 1 || t[4] < 1 || t[6] >= H || t[7] >= W) continue;
        const int64_t z = r / H, y = r - z * H;
        if (y < 1 || y + 1 >= H) continue;
        const T *src = lab + r * W;
        const T *rows[4] = {src - W, src + W, z > 0 ? src - H * W : (below ? below + y * W : nullptr),
                            z + 1 < D ? src + H * W : (above ? above + y * W : nullptr)};
        uint32_t mn = 0xffffffffu, mx = 0u;                  // a wall label is non-zero, so mx == 0: none seen
        if (sub == 0) {
            const uint32_t u = (uint32_t)src[a0 - 1], v = (uint32_t)src[a1];
            mn = min(u, v);
            mx = max(u, v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const T *p = rows[q];
            if (p == nullptr) continue;
            for (int64_t x = a0 + sub; x < a1; x += 16) {
                const uint32_t v = (uint32_t)p[x];
                if (v != 0u) {
                    mn = min(mn, v);
                    mx = max(mx, v);
                }
            }
        }
        if (mx != 0u) {
            unsigned long long *u = reinterpret_cast<unsigned long long *>(t);
            if ((unsigned long long)mn < u[8]) atomicMin(u + 8, (unsigned long long)mn);
            if ((unsigned long long)mx > u[9]) atomicMax(u + 9, (unsigned long long)mx);
        }
    }
}

// same shape checks as emp_measure.hip: one run per voxel is the worst case and the scan is int32
#define HL_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                             \
        EMP_REQUIRE_LABELS(what);                                                                                    \
        EMP_REQUIRE(H <= 0x7fffffffLL / W && (D == 0 || H * W <= 0x7fffffffLL / D),                                  \
                    what ": %lld x %lld x %lld voxels could hold more than 2^31 - 1 runs; cut the slab into z-blocks", \
                    (long long)D, (long long)H, (long long)W);                                                       \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0, what ": misaligned labels");          \
    } while (0)

// ------------------------------------------------------------------------------------------ count + scan
extern "C" int64_t emp_label_holes_count_work_bytes(int64_t R) { return emp_count_carve(nullptr, R).total; }

template <typename T, bool EXTRACT>
static int hl_launch_rows(const void *lab, int64_t n_rows, int64_t W, int32_t *row_counts, const int32_t *row_offsets,
                          int64_t n_runs, const CcWork &L, hipStream_t st)
{
    EMP_LAUNCH((hl_rows_kernel<T, EXTRACT>), emp_grid(n_rows * 64, 256, 16384), 256, st,
               reinterpret_cast<const T *>(lab), n_rows, W, row_counts, row_offsets, n_runs, L.row, L.xs, L.xe);
    return EMP_OK;
}

extern "C" int emp_label_holes_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, void *work,
                                     int64_t work_bytes, int32_t *row_offsets, void *stream)
{
    HL_REQUIRE_SHAPE("label_holes_count");
    EMP_REQUIRE(work && row_offsets, "label_holes_count: null pointer");
    const int64_t R = D * H;
    EmpCountWork C = emp_count_carve(work, R);
    EMP_REQUIRE(work_bytes >= C.total, "label_holes_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)C.total);
    hipStream_t st = emp_stream(stream);
    if (R == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, row_offsets, (int64_t)1);
        return EMP_OK;
    }
    const CcWork none = {};
    int rc = item == 4 ? hl_launch_rows<uint32_t, false>(lab, R, W, C.counts, nullptr, 0, none, st)
                       : hl_launch_rows<uint8_t, false>(lab, R, W, C.counts, nullptr, 0, none, st);
    if (rc != EMP_OK) return rc;
    return emp_exclusive_scan_i32(C.counts, R, row_offsets, C.scantmp, stream);
}

// ------------------------------------------------------------------------------------------ extract + unite + table
extern "C" int64_t emp_label_holes_work_bytes(int64_t n_runs) { return cc_carve(nullptr, n_runs).total; }

extern "C" int emp_label_holes(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                               const void *above, int64_t z_base, const int32_t *row_offsets, int64_t n_runs,
                               void *work, int64_t work_bytes, int64_t *out_table, int32_t *n_out, void *stream)
{
    HL_REQUIRE_SHAPE("label_holes");
    EMP_REQUIRE(row_offsets && n_out, "label_holes: null pointer");
    EMP_REQUIRE((!below || reinterpret_cast<uintptr_t>(below) % (uintptr_t)item == 0) &&
                (!above || reinterpret_cast<uintptr_t>(above) % (uintptr_t)item == 0),
                "label_holes: misaligned neighbour slice");
    EMP_REQUIRE(z_base >= 0 && z_base <= (1LL << 40), "label_holes: z_base = %lld outside 0 .. 2^40",
                (long long)z_base);
    EMP_REQUIRE(n_runs >= 0 && n_runs <= D * H * W, "label_holes: n_runs = %lld is not the run total of %lld voxels",
                (long long)n_runs, (long long)(D * H * W));
    hipStream_t st = emp_stream(stream);
    if (n_runs == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_out, (int64_t)1);
        return EMP_OK;
    }
    EMP_REQUIRE(work && out_table, "label_holes: null pointer");
    CcWork L = cc_carve(work, n_runs);
    EMP_REQUIRE(work_bytes >= L.total, "label_holes: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    // every run's value is 0, which is what the paint step compares a lut entry with; a slot that the extraction does
    // not reach (labels changed since step 1) reads as an empty run of row 0
    EMP_LAUNCH(emp_zero_kernel<int32_t>, emp_grid(L.keep / 4, 256, 4096), 256, st, L.row, L.keep / 4);
    int rc = item == 4 ? hl_launch_rows<uint32_t, true>(lab, D * H, W, nullptr, row_offsets, n_runs, L, st)
                       : hl_launch_rows<uint8_t, true>(lab, D * H, W, nullptr, row_offsets, n_runs, L, st);
    if (rc != EMP_OK) return rc;
    rc = emp_cc_unite(L, n_runs, H, D * H, 6, row_offsets, stream);
    if (rc != EMP_OK) return rc;
    const int grid = emp_grid(n_runs, 256, 4096);
    rc = emp_compact(
        L.flag, n_runs, L.pos, L.scantmp, n_out, stream, "label_holes: count copy",
        [&]() -> int { return emp_cc_roots(L, n_runs, stream); },
        [&]() -> int {
            EMP_LAUNCH(hl_comp_kernel, grid, 256, st, n_runs, W, z_base * H * W, L.parent, L.flag, L.pos, L.row, L.xs,
                       L.comp, out_table);
            return EMP_OK;
        });
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(hl_stats_kernel, emp_grid(emp_cdiv(n_runs, HL_SEG), 256, 4096), 256, st, n_runs, H, z_base, L.row, L.xs,
               L.xe, L.comp, out_table);
    const int sgrid = emp_grid(n_runs * 16, 256, 8192);
    if (item == 4)
        EMP_LAUNCH((hl_survey_kernel<uint32_t>), sgrid, 256, st, n_runs, D, H, W, reinterpret_cast<const uint32_t *>(lab),
                   reinterpret_cast<const uint32_t *>(below), reinterpret_cast<const uint32_t *>(above), L.row, L.xs,
                   L.xe, L.comp, out_table);
    else
        EMP_LAUNCH((hl_survey_kernel<uint8_t>), sgrid, 256, st, n_runs, D, H, W, reinterpret_cast<const uint8_t *>(lab),
                   reinterpret_cast<const uint8_t *>(below), reinterpret_cast<const uint8_t *>(above), L.row, L.xs, L.xe,
                   L.comp, out_table);
    return EMP_OK;
}
