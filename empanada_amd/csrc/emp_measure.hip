// Per-object measurements of a label volume (include/emp_hip.h, E2): one row per distinct non-zero label with its voxel
// count, bounding box, index sums and exposed faces.  No counterpart in the reference, whose trackers carry boxes and
// runs per plane only (inference/tracker.py:61-123); the definition is the header's.
//
// Same two-phase shape as emp_overlaps.hip: count the runs of one non-zero label per row (ballots + a carried last
// voxel), scan the row counts, extract one record per run to row_offset + i, sort the records by label, fold equal
// labels.  A run of length n at (z, y, xs) adds n voxels, n z, n y, n xs + n (n - 1) / 2 to the sums and 2 faces normal
// to x; its faces normal to y and z are the sum over its voxels of the neighbours (y +- 1, z +- 1) that differ, read
// off an inclusive scan of that per-voxel count carried along the row: the exclusive value at the run's start, the
// inclusive value at its end.  Everything after the two voxel passes is O(#runs), and no table is sized by a guess.
#include "emp_common.h"

// ------------------------------------------------------------------------------------------ runs of one label per row
// One wave per row; each lane owns 4 consecutive voxels.  As in ov_spans_kernel the lane grid of a row starts at -shift,
// shift = (element index of the row's first voxel) mod 4, so that every full group of the row is one aligned load (16
// bytes of uint32, 4 bytes of uint8) for ANY W and any base offset.  A group cut by the row's ends, and a group of a
// neighbour row that does not start on such an address (W no multiple of 4, or neighbour slices at another offset), is
// read voxel by voxel: the narrow path, same values.  A null row and positions outside the row read as 0.
// the run records of a call, indexed by run (row_offsets[row] + position in the row)
struct MsRuns {
    uint64_t *key;                 // label
    int32_t *idx;                  // the run's own index: the value that travels through the sort
    int32_t *row, *xs, *xe;        // xe: exclusive end, made a length by ms_fix_kernel
    uint32_t *ey0, *ey1, *ez0, *ez1;  // carried exposure scans: exclusive at the start, inclusive at the end
    uint32_t *val;                 // the label as it is, written in place of key / idx / exposures without EXPOSE
};

// EXPOSE (the measurements) reads the four neighbour rows and carries the exposure scans; an extraction without it
// (emp_components.hip) reads the centre row alone and records (row, xs, xe, val) per run.
template <typename T, bool EXTRACT, bool EXPOSE = EXTRACT>
__global__ __launch_bounds__(256) void ms_rows_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                      const T *__restrict__ below, const T *__restrict__ above,
                                                      int32_t *__restrict__ row_counts,
                                                      const int32_t *__restrict__ row_offsets, int64_t n_runs, MsRuns r)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_rows = D * H;
    const unsigned long long before = (1ull << lane) - 1ull;            // lanes before this one
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        const int64_t z = row / H, y = row - z * H;
        const T *src = lab + row * W;
        const int shift = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & 3);
        // the four neighbour rows: inside the block, the neighbour slices at its two ends, nothing outside
        const T *ym = nullptr, *yp = nullptr, *zm = nullptr, *zp = nullptr;
        if (EXPOSE) {
            ym = y > 0 ? src - W : nullptr;
            yp = y + 1 < H ? src + W : nullptr;
            zm = z > 0 ? src - H * W : (below ? below + y * W : nullptr);
            zp = z + 1 < D ? src + H * W : (above ? above + y * W : nullptr);
        }
        int n_s = 0, n_e = 0;  // wave-uniform running counts of starts / ends in this row
        const int32_t obase = EXTRACT ? row_offsets[row] : 0;
        uint32_t c[4], nx[4];
        emp_fetch4<T>(src, (int64_t)lane * 4 - shift, W, c);
        uint32_t carry = 0u;                                            // voxel left of the chunk (0 at the row start)
        uint32_t sy = 0u, sz = 0u;                                      // exposure sums of the row before this chunk
        for (int64_t x0 = -shift; x0 < W; x0 += 256) {
            const int64_t x = x0 + (int64_t)lane * 4;
            // the next chunk is requested before this one is scanned
            if (x0 + 256 < W) emp_fetch4<T>(src, x + 256, W, nx);
            else nx[0] = nx[1] = nx[2] = nx[3] = 0u;
            // a chunk of background alone (wave uniform) starts and ends nothing -- a run that ended on the voxel before
            // it was closed there, against this chunk's first voxel -- and does not wait for the chunk after it
            if (__ballot((c[0] | c[1] | c[2] | c[3]) != 0u) == 0ull) {
                carry = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = nx[j];
                continue;
            }
            // only a lane that holds a non-zero voxel reads the neighbour rows, so background costs the centre row alone;
            // the four loads go out before anything waits for the next chunk
            uint32_t a[4] = {0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u}, f[4] = {0u, 0u, 0u, 0u}, g[4] = {0u, 0u, 0u, 0u};
            if (EXPOSE && (c[0] | c[1] | c[2] | c[3]) != 0u) {
                emp_fetch4<T>(ym, x, W, a);
                emp_fetch4<T>(yp, x, W, b);
                emp_fetch4<T>(zm, x, W, f);
                emp_fetch4<T>(zp, x, W, g);
            }
            uint32_t left = __shfl_up(c[3], 1), right = __shfl_down(c[0], 1);
            const uint32_t first_next = __shfl(nx[0], 0);
            if (lane == 0) left = carry;
            if (lane == 63) right = first_next;                         // 0 past the row's end
            const uint32_t v[6] = {left, c[0], c[1], c[2], c[3], right};
            bool st[4], en[4];
            unsigned long long bs[4], be[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                st[j] = v[j + 1] != 0u && v[j + 1] != v[j];
                en[j] = v[j + 1] != 0u && v[j + 1] != v[j + 2];
                bs[j] = __ballot(st[j]);
                be[j] = __ballot(en[j]);
            }
            int tot_s = 0, tot_e = 0, ps = 0, pe = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                tot_s += __popcll(bs[j]);
                tot_e += __popcll(be[j]);
                if (EXTRACT) {
                    ps += __popcll(bs[j] & before);
                    pe += __popcll(be[j] & before);
                }
            }
            if (EXTRACT) {
                // per-voxel exposure, y in the low half and z in the high half: at most 2 each, 512 each per chunk
                uint32_t e[4] = {0u, 0u, 0u, 0u};
                uint32_t incl = 0u, p = 0u;
                if (EXPOSE) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        e[j] = c[j] == 0u ? 0u
                                          : (uint32_t)(c[j] != a[j]) + (uint32_t)(c[j] != b[j]) +
                                                (((uint32_t)(c[j] != f[j]) + (uint32_t)(c[j] != g[j])) << 16);
                    const uint32_t lane_tot = e[0] + e[1] + e[2] + e[3];
                    incl = lane_tot;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t t = __shfl_up(incl, d);
                        if (lane >= d) incl += t;
                    }
                    p = incl - lane_tot;                                // exposure of the chunk before this lane
                }
                int is = obase + n_s + ps, ie = obase + n_e + pe;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (st[j]) {
                        if (is < n_runs) {
                            r.row[is] = (int32_t)row;
                            r.xs[is] = (int32_t)(x + j);
                            if (EXPOSE) {
                                r.key[is] = (uint64_t)c[j];
                                r.idx[is] = is;
                                r.ey0[is] = sy + (p & 0xffffu);
                                r.ez0[is] = sz + (p >> 16);
                            } else {
                                r.val[is] = c[j];
                            }
                        }
                        ++is;
                    }
                    p += e[j];
                    if (en[j]) {
                        if (ie < n_runs) {
                            r.xe[ie] = (int32_t)(x + j + 1);
                            if (EXPOSE) {
                                r.ey1[ie] = sy + (p & 0xffffu);
                                r.ez1[ie] = sz + (p >> 16);
                            }
                        }
                        ++ie;
                    }
                }
                if (EXPOSE) {
                    const uint32_t chunk_tot = __shfl(incl, 63);
                    sy += chunk_tot & 0xffffu;                          // at most 2 W < 2^32 over a row
                    sz += chunk_tot >> 16;
                }
            }
            n_s += tot_s;
            n_e += tot_e;
            carry = __shfl(c[3], 63);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = nx[j];
        }
        if (!EXTRACT && lane == 0) row_counts[row] = n_s;
    }
}

// ends -> lengths, scan pairs -> exposures of the run
__global__ void ms_fix_kernel(MsRuns r, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        r.xe[i] -= r.xs[i];
        r.ey0[i] = r.ey1[i] - r.ey0[i];
        r.ez0[i] = r.ez1[i] - r.ez0[i];
    }
}

#define MS_COLS 14
// sums and maxima start at 0, minima at the largest int64
__global__ void ms_init_kernel(int64_t *__restrict__ table, int64_t n_rows)
{
    const int64_t n = n_rows * MS_COLS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % MS_COLS);
        table[i] = (col >= 2 && col <= 4) ? 0x7fffffffffffffffLL : 0LL;
    }
}

// what one thread has folded of one label; every value is a non-negative integer
struct MsAcc {
    unsigned long long vox, sz, sy, sx, fz, fy, fx, z0, y0, x0, z1, y1, x1;
    __device__ void reset()
    {
        vox = sz = sy = sx = fz = fy = fx = z1 = y1 = x1 = 0ull;
        z0 = y0 = x0 = ~0ull;
    }
    __device__ void flush(int64_t *__restrict__ row) const
    {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(row);
        atomicAdd(o + 1, vox);
        atomicMin(o + 2, z0);
        atomicMin(o + 3, y0);
        atomicMin(o + 4, x0);
        atomicMax(o + 5, z1);
        atomicMax(o + 6, y1);
        atomicMax(o + 7, x1);
        atomicAdd(o + 8, sz);
        atomicAdd(o + 9, sy);
        atomicAdd(o + 10, sx);
        atomicAdd(o + 11, fz);
        atomicAdd(o + 12, fy);
        atomicAdd(o + 13, fx);
    }
};

// As ov_reduce_kernel, every thread folds MS_SEG consecutive sorted runs and sends what it has of a label to the label's
// row where the label changes inside its segment.  What it holds at the segment's end is first combined over the wave:
// the runs are sorted, so the lanes that end in one label are neighbours, a segmented scan (6 shuffle steps) adds them
// up, and the last lane of every such group alone issues the atomics.  A label with a million runs -- the one label of
// a stuff class -- then costs 1 / (64 MS_SEG) as many atomics on its row.  Integer add / min / max: neither the order
// of the atomics nor the grouping shows.
#define MS_SEG 16
__device__ __forceinline__ unsigned long long ms_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long ms_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__global__ __launch_bounds__(256) void ms_reduce_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ idx,
                                                        int64_t n, const int32_t *__restrict__ head,
                                                        const int32_t *__restrict__ pos, MsRuns r, int64_t H,
                                                        int64_t z_base, int64_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_seg = (n + MS_SEG - 1) / MS_SEG;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // the whole wave walks together (base is wave uniform), so that every lane takes part in the shuffles
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n_seg; base += stride) {
        const int64_t s = base + lane;
        int64_t o = -1;                                      // a lane past the last segment: no label, nothing to send
        MsAcc a;
        a.reset();
        if (s < n_seg) {
            const int64_t i0 = s * MS_SEG, i1 = (i0 + MS_SEG < n) ? i0 + MS_SEG : n;
            o = (int64_t)pos[i0] - (head[i0] ? 0 : 1);       // pos counts the heads BEFORE i: a run inside a label sits one
                                                             // past its own head
            for (int64_t i = i0; i < i1; ++i) {
                if (head[i]) {
                    if (i != i0) {
                        a.flush(out + o * MS_COLS);
                        a.reset();
                        o = pos[i];
                    }
                    out[o * MS_COLS] = (int64_t)(keys[i] & 0xffffffffULL);
                }
                const int32_t k = idx[i];
                const int64_t row = r.row[k];
                const unsigned long long zl = (unsigned long long)(row / H);
                const unsigned long long y = (unsigned long long)row - zl * (unsigned long long)H;
                const unsigned long long z = zl + (unsigned long long)z_base;
                const unsigned long long xs = (unsigned long long)r.xs[k], len = (unsigned long long)r.xe[k];
                a.vox += len;
                a.sz += len * z;
                a.sy += len * y;
                a.sx += len * xs + len * (len - 1ull) / 2ull;
                a.fz += (unsigned long long)r.ez0[k];
                a.fy += (unsigned long long)r.ey0[k];
                a.fx += 2ull;
                a.z0 = ms_min(a.z0, z);
                a.y0 = ms_min(a.y0, y);
                a.x0 = ms_min(a.x0, xs);
                a.z1 = ms_max(a.z1, z + 1ull);
                a.y1 = ms_max(a.y1, y + 1ull);
                a.x1 = ms_max(a.x1, xs + len);
            }
        }
        // segmented inclusive scan over the lanes by output row: rows ascend along the wave, so a lane d below with the
        // same row means every lane between holds that row too
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t po = __shfl_up(o, d);
            MsAcc b;
            b.vox = __shfl_up(a.vox, d); b.sz = __shfl_up(a.sz, d); b.sy = __shfl_up(a.sy, d); b.sx = __shfl_up(a.sx, d);
            b.fz = __shfl_up(a.fz, d); b.fy = __shfl_up(a.fy, d); b.fx = __shfl_up(a.fx, d);
            b.z0 = __shfl_up(a.z0, d); b.y0 = __shfl_up(a.y0, d); b.x0 = __shfl_up(a.x0, d);
            b.z1 = __shfl_up(a.z1, d); b.y1 = __shfl_up(a.y1, d); b.x1 = __shfl_up(a.x1, d);
            if (lane >= d && po == o) {
                a.vox += b.vox; a.sz += b.sz; a.sy += b.sy; a.sx += b.sx; a.fz += b.fz; a.fy += b.fy; a.fx += b.fx;
                a.z0 = ms_min(a.z0, b.z0); a.y0 = ms_min(a.y0, b.y0); a.x0 = ms_min(a.x0, b.x0);
                a.z1 = ms_max(a.z1, b.z1); a.y1 = ms_max(a.y1, b.y1); a.x1 = ms_max(a.x1, b.x1);
            }
        }
        const int64_t no = __shfl_down(o, 1);
        if (o >= 0 && (lane == 63 || no != o)) a.flush(out + o * MS_COLS);
    }
}

// shared argument checks of the two entry points; the run total of a call is at most one per voxel, so D * H * W inside
// int32 keeps the scan's int32 total exact whatever the labels are
#define MS_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                             \
        EMP_REQUIRE_LABELS(what);                                                                                    \
        EMP_REQUIRE(H <= 0x7fffffffLL / W && (D == 0 || H * W <= 0x7fffffffLL / D),                                  \
                    what ": %lld x %lld x %lld voxels could hold more than 2^31 - 1 runs; cut the slab into z-blocks", \
                    (long long)D, (long long)H, (long long)W);                                                       \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0, what ": misaligned labels");          \
    } while (0)

// ------------------------------------------------------------------------------------------ count + scan
extern "C" int64_t emp_label_measure_count_work_bytes(int64_t R) { return emp_count_carve(nullptr, R).total; }

template <typename T, bool EXTRACT, bool EXPOSE = EXTRACT>
static int ms_launch(const void *lab, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                     int32_t *row_counts, const int32_t *row_offsets, int64_t n_runs, const MsRuns &r, hipStream_t st)
{
    EMP_LAUNCH((ms_rows_kernel<T, EXTRACT, EXPOSE>), emp_grid(D * H * 64, 256, 16384), 256, st, reinterpret_cast<const T *>(lab),
               D, H, W, reinterpret_cast<const T *>(below), reinterpret_cast<const T *>(above), row_counts, row_offsets,
               n_runs, r);
    return EMP_OK;
}

extern "C" int emp_label_measure_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, void *work,
                                       int64_t work_bytes, int32_t *row_offsets, void *stream)
{
    MS_REQUIRE_SHAPE("label_measure_count");
    EMP_REQUIRE(work && row_offsets, "label_measure_count: null pointer");
    const int64_t R = D * H;
    EmpCountWork L = emp_count_carve(work, R);
    EMP_REQUIRE(work_bytes >= L.total, "label_measure_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    if (R == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, row_offsets, (int64_t)1);
        return EMP_OK;
    }
    const MsRuns none = {};
    int rc = item == 4 ? ms_launch<uint32_t, false>(lab, D, H, W, nullptr, nullptr, L.counts, nullptr, 0, none, st)
                       : ms_launch<uint8_t, false>(lab, D, H, W, nullptr, nullptr, L.counts, nullptr, 0, none, st);
    if (rc != EMP_OK) return rc;
    return emp_exclusive_scan_i32(L.counts, R, row_offsets, L.scantmp, stream);
}

// The runs of step 1's definition as (row, x start, exclusive x end, label) at row_offsets[row] + position in the row,
// for emp_components.hip: the same kernel without the neighbour rows.  The caller has checked the shape.
int emp_label_rows_extract(const void *lab, int item, int64_t D, int64_t H, int64_t W, const int32_t *row_offsets,
                           int64_t n_runs, int32_t *row, int32_t *xs, int32_t *xe, uint32_t *val, void *stream)
{
    MsRuns r = {};
    r.row = row;
    r.xs = xs;
    r.xe = xe;
    r.val = val;
    hipStream_t st = emp_stream(stream);
    return item == 4 ? ms_launch<uint32_t, true, false>(lab, D, H, W, nullptr, nullptr, nullptr, row_offsets, n_runs, r, st)
                     : ms_launch<uint8_t, true, false>(lab, D, H, W, nullptr, nullptr, nullptr, row_offsets, n_runs, r, st);
}

// ------------------------------------------------------------------------------------------ extract + sort + reduce
struct MsWork {
    uint64_t *keys_out;
    int32_t *idx_out, *head, *pos, *scantmp;
    MsRuns r;
    char *cub;
    int64_t cub_bytes, total;
};
static MsWork ms_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    MsWork L;
    L.r.key = c.take<uint64_t>(n);
    L.keys_out = c.take<uint64_t>(n);
    L.r.idx = c.take<int32_t>(n);
    L.idx_out = c.take<int32_t>(n);
    L.r.row = c.take<int32_t>(n);
    L.r.xs = c.take<int32_t>(n);
    L.r.xe = c.take<int32_t>(n);
    L.r.ey0 = c.take<uint32_t>(n);
    L.r.ez0 = c.take<uint32_t>(n);
    L.head = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    // the inclusive ends of the exposure scans are dead (ms_fix_kernel) before the heads and positions are written
    L.r.ey1 = reinterpret_cast<uint32_t *>(L.head);
    L.r.ez1 = reinterpret_cast<uint32_t *>(L.pos);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.cub_bytes = emp_sort_work_bytes(n);
    L.cub = c.take<char>(L.cub_bytes);
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_label_measure_work_bytes(int64_t n_runs) { return ms_carve(nullptr, n_runs).total; }

extern "C" int emp_label_measure(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                 const void *above, int64_t z_base, const int32_t *row_offsets, int64_t n_runs,
                                 void *work, int64_t work_bytes, int64_t *out_table, int32_t *n_out, void *stream)
{
    MS_REQUIRE_SHAPE("label_measure");
    EMP_REQUIRE(row_offsets && n_out, "label_measure: null pointer");
    EMP_REQUIRE((!below || reinterpret_cast<uintptr_t>(below) % (uintptr_t)item == 0) &&
                (!above || reinterpret_cast<uintptr_t>(above) % (uintptr_t)item == 0),
                "label_measure: misaligned neighbour slice");
    EMP_REQUIRE(z_base >= 0 && z_base <= (1LL << 40), "label_measure: z_base = %lld outside 0 .. 2^40",
                (long long)z_base);
    EMP_REQUIRE(n_runs >= 0 && n_runs <= D * H * W, "label_measure: n_runs = %lld is not the run total of %lld voxels",
                (long long)n_runs, (long long)(D * H * W));
    hipStream_t st = emp_stream(stream);
    if (n_runs == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_out, (int64_t)1);
        return EMP_OK;
    }
    EMP_REQUIRE(work && out_table, "label_measure: null pointer");
    MsWork L = ms_carve(work, n_runs);
    EMP_REQUIRE(work_bytes >= L.total, "label_measure: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    const int grid = emp_grid(n_runs, 256, 4096);
    int rc = item == 4 ? ms_launch<uint32_t, true>(lab, D, H, W, below, above, nullptr, row_offsets, n_runs, L.r, st)
                       : ms_launch<uint8_t, true>(lab, D, H, W, below, above, nullptr, row_offsets, n_runs, L.r, st);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(ms_fix_kernel, grid, 256, st, L.r, n_runs);
    rc = emp_sort_u64_i32(L.r.key, L.keys_out, L.r.idx, L.idx_out, n_runs, 0, 32, L.cub, L.cub_bytes, stream);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(ms_init_kernel, emp_grid(n_runs * MS_COLS, 256, 4096), 256, st, out_table, n_runs);
    return emp_compact(
        L.head, n_runs, L.pos, L.scantmp, n_out, stream, "label_measure: count copy",
        [&]() -> int {
            EMP_LAUNCH(emp_heads_kernel<0>, grid, 256, st, L.keys_out, n_runs, L.head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(ms_reduce_kernel, emp_grid(emp_cdiv(n_runs, MS_SEG), 256, 4096), 256, st, L.keys_out, L.idx_out,
                       n_runs, L.head, L.pos, L.r, H, z_base, out_table);
            return EMP_OK;
        });
}
