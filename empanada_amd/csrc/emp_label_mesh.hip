// Surface meshes of a label volume (include/emp_hip.h, E7): one welded, outward-oriented quad mesh per non-zero label,
// made of the voxel faces that E2 calls exposed.  What users of the reference do on a CPU afterwards, object by object,
// with skimage.measure.marching_cubes or zmesh; the definition is the header's.
//
// Count -> scan -> emit, as emp_measure.hip: one wave per row, each lane owns 4 consecutive positions, the lane grid of a
// row starts on an aligned address, a chunk of background alone is left at once.  There are two kinds of rows.  A VOXEL
// row (z, y) emits the quads of its voxels: up to six per voxel, in the order (x, direction code).  A CORNER row
// (z, y) of an owned corner plane emits one key, label << 32 | corner number, for every distinct label among the eight
// voxels around each of its W + 1 corners, unless that label fills all eight.  Both kinds go through ONE kernel and ONE
// scan: rows 0 .. D H - 1 are the voxel rows, the corner rows follow, so row_offsets[D H] is the quad total and
// row_offsets[R] - row_offsets[D H] the key total.  No atomics anywhere: every output position is a prefix sum.
//
// The host sorts the keys (all 64 bits) and the quads (label bits only, stable) with emp_sort_u64_i32; lm_index then
// cuts the sorted keys into objects, unpacks them into vertices and resolves every quad corner by a binary search
// inside its object's own range of the keys.  Smoothing gathers over a six-slot neighbour table.
#include "emp_common.h"

template <typename T>
__device__ __forceinline__ uint32_t lm_one(const T *__restrict__ src, int64_t x, int64_t W)
{
    return (src != nullptr && x >= 0 && x < W) ? (uint32_t)src[x] : 0u;
}

// inclusive sum over the wave
__device__ __forceinline__ int lm_wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// The vertices of one corner: the distinct non-zero labels among its eight voxels, none if one value fills all eight.
// EMIT writes label << 32 | corner for each to keys[pos ..), never at or past n_keys; returns how many there are.
template <bool EMIT>
__device__ __forceinline__ int lm_corner(const uint32_t (&v)[8], uint64_t corner, uint64_t *__restrict__ keys, int64_t pos,
                                         int64_t n_keys)
{
    bool same = true;
#pragma unroll
    for (int j = 1; j < 8; ++j) same = same && v[j] == v[0];
    if (same) return 0;
    int n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool fresh = v[j] != 0u;
#pragma unroll
        for (int k = 0; k < j; ++k) fresh = fresh && v[k] != v[j];
        if (fresh) {
            if (EMIT && pos + n < n_keys) keys[pos + n] = ((uint64_t)v[j] << 32) | corner;
            ++n;
        }
    }
    return n;
}

struct LmOut {
    uint64_t *vkeys;   // label << 32 | corner, one per vertex the block owns, in corner order
    uint64_t *qkeys;   // label << 32 | the quad's lowest corner, in (z, y, x, direction) order
    int32_t *qdirs;    // direction code of the quad: -z 0, +z 1, -y 2, +y 3, -x 4, +x 5
    int64_t n_quads, n_keys;
};

template <typename T, bool EMIT>
__global__ __launch_bounds__(256) void lm_rows_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                      const T *__restrict__ below, const T *__restrict__ above, int top,
                                                      int64_t z_base, int32_t *__restrict__ row_counts,
                                                      const int32_t *__restrict__ row_offsets, LmOut o)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_vrows = D * H, n_rows = n_vrows + (D + (top ? 1 : 0)) * (H + 1);
    const uint64_t ey = (uint64_t)(W + 1), ez = (uint64_t)(H + 1) * ey;         // corner steps along y and z (x: 1)
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        int run = 0;                                                            // wave uniform: items of the row so far
        if (row < n_vrows) {
            // ------------------------------------------------------------------ the quads of a voxel row
            const int64_t z = row / H, y = row - z * H;
            const T *src = lab + row * W;
            const int shift = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & 3);
            const T *ym = y > 0 ? src - W : nullptr;
            const T *yp = y + 1 < H ? src + W : nullptr;
            const T *zm = z > 0 ? src - H * W : (below ? below + y * W : nullptr);
            const T *zp = z + 1 < D ? src + H * W : (above ? above + y * W : nullptr);
            const int64_t obase = EMIT ? (int64_t)row_offsets[row] : 0;
            const uint64_t c0 = (uint64_t)(z_base + z) * ez + (uint64_t)y * ey;  // corner (z, y, 0) of the voxel row
            for (int64_t x0 = -shift; x0 < W; x0 += 256) {
                const int64_t x = x0 + (int64_t)lane * 4;
                uint32_t c[4];
                emp_fetch4<T>(src, x, W, c);
                const bool any = (c[0] | c[1] | c[2] | c[3]) != 0u;
                if (__ballot(any) == 0ull) continue;                            // background alone owns no quad
                // only a lane that holds a non-zero voxel reads the neighbour rows
                uint32_t a[4] = {0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u}, f[4] = {0u, 0u, 0u, 0u}, g[4] = {0u, 0u, 0u, 0u};
                if (any) {
                    emp_fetch4<T>(ym, x, W, a);
                    emp_fetch4<T>(yp, x, W, b);
                    emp_fetch4<T>(zm, x, W, f);
                    emp_fetch4<T>(zp, x, W, g);
                }
                uint32_t left = __shfl_up(c[3], 1), right = __shfl_down(c[0], 1);
                if (lane == 0) left = lm_one<T>(src, x - 1, W);
                if (lane == 63) right = lm_one<T>(src, x + 4, W);
                const uint32_t v[6] = {left, c[0], c[1], c[2], c[3], right};
                uint32_t mask[4];
                int lane_tot = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    mask[j] = c[j] == 0u ? 0u
                                         : (uint32_t)(c[j] != f[j]) | ((uint32_t)(c[j] != g[j]) << 1) |
                                               ((uint32_t)(c[j] != a[j]) << 2) | ((uint32_t)(c[j] != b[j]) << 3) |
                                               ((uint32_t)(c[j] != v[j]) << 4) | ((uint32_t)(c[j] != v[j + 2]) << 5);
                    lane_tot += __popc(mask[j]);
                }
                const int incl = lm_wave_scan(lane_tot, lane);
                if (EMIT) {
                    int64_t p = obase + run + (incl - lane_tot);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint64_t lo = c0 + (uint64_t)(x + j);             // the voxel's lowest corner
                        const uint64_t step[6] = {0ull, ez, 0ull, ey, 0ull, 1ull};
#pragma unroll
                        for (int d = 0; d < 6; ++d) {
                            if ((mask[j] >> d) & 1u) {
                                if (p < o.n_quads) {
                                    o.qkeys[p] = ((uint64_t)c[j] << 32) | (lo + step[d]);
                                    o.qdirs[p] = d;
                                }
                                ++p;
                            }
                        }
                    }
                }
                run += __shfl(incl, 63);
            }
        } else {
            // ------------------------------------------------------------------ the vertices of a corner row
            const int64_t cr = row - n_vrows;
            const int64_t zc = cr / (H + 1), yc = cr - zc * (H + 1);
            // voxel slices zc - 1 and zc, voxel rows yc - 1 and yc: inside the block, the neighbour slices, nothing
            const T *s0 = zc > 0 ? lab + (zc - 1) * H * W : below;
            const T *s1 = zc < D ? lab + zc * H * W : above;
            const T *r[4];
            r[0] = (s0 && yc > 0) ? s0 + (yc - 1) * W : nullptr;
            r[1] = (s0 && yc < H) ? s0 + yc * W : nullptr;
            r[2] = (s1 && yc > 0) ? s1 + (yc - 1) * W : nullptr;
            r[3] = (s1 && yc < H) ? s1 + yc * W : nullptr;
            const T *first = r[0] ? r[0] : r[1] ? r[1] : r[2] ? r[2] : r[3];
            if (first != nullptr) {
                const int shift = (int)((reinterpret_cast<uintptr_t>(first) / sizeof(T)) & 3);
                const int64_t obase = EMIT ? (int64_t)row_offsets[row] - (int64_t)row_offsets[n_vrows] : 0;
                const uint64_t c0 = (uint64_t)(z_base + zc) * ez + (uint64_t)yc * ey;
                for (int64_t x0 = -shift; x0 <= W; x0 += 256) {                 // corners 0 .. W
                    const int64_t x = x0 + (int64_t)lane * 4;
                    uint32_t q[4][5];                                           // voxels x - 1 .. x + 3 of the four rows
                    uint32_t any = 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        emp_fetch4<T>(r[k], x, W, &q[k][1]);
                        q[k][0] = __shfl_up(q[k][4], 1);
                        if (lane == 0) q[k][0] = lm_one<T>(r[k], x - 1, W);
                        any |= q[k][0] | q[k][1] | q[k][2] | q[k][3] | q[k][4];
                    }
                    if (__ballot(any != 0u) == 0ull) continue;
                    // corner x + j sees voxels x + j - 1 and x + j of every row; outside 0 .. W both read 0: no vertex
                    int cnt[4] = {0, 0, 0, 0};
                    if (any != 0u) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t v[8] = {q[0][j], q[0][j + 1], q[1][j], q[1][j + 1],
                                                   q[2][j], q[2][j + 1], q[3][j], q[3][j + 1]};
                            cnt[j] = lm_corner<false>(v, 0ull, nullptr, 0, 0);
                        }
                    }
                    const int lane_tot = cnt[0] + cnt[1] + cnt[2] + cnt[3];
                    const int incl = lm_wave_scan(lane_tot, lane);
                    if (EMIT && lane_tot != 0) {
                        int64_t p = obase + run + (incl - lane_tot);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (cnt[j] != 0) {
                                const uint32_t v[8] = {q[0][j], q[0][j + 1], q[1][j], q[1][j + 1],
                                                       q[2][j], q[2][j + 1], q[3][j], q[3][j + 1]};
                                p += lm_corner<true>(v, c0 + (uint64_t)(x + j), o.vkeys, p, o.n_keys);
                            }
                        }
                    }
                    run += __shfl(incl, 63);
                }
            }
        }
        if (!EMIT && lane == 0) row_counts[row] = run;
    }
}

// ------------------------------------------------------------------------------------------ entry points: count, emit
// A block emits at most 6 quads per voxel and 8 keys per voxel of the D + 2 slices it sees (a key needs a voxel of its
// label at the corner), so D H W <= 2^26 keeps the total, at most (6 D + 8 (D + 2)) H W < 2^31, inside the int32 scan.
#define LM_MAX_VOXELS (1LL << 26)
#define LM_REQUIRE_SHAPE(what)                                                                                        \
    do {                                                                                                              \
        EMP_REQUIRE_LABELS(what);                                                                                     \
        EMP_REQUIRE(H <= LM_MAX_VOXELS / W && (D == 0 || H * W <= LM_MAX_VOXELS / D),                                 \
                    what ": %lld x %lld x %lld voxels exceed 2^26 per call; cut the slab into z-blocks",              \
                    (long long)D, (long long)H, (long long)W);                                                        \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 &&                                      \
                        (!below || reinterpret_cast<uintptr_t>(below) % (uintptr_t)item == 0) &&                      \
                        (!above || reinterpret_cast<uintptr_t>(above) % (uintptr_t)item == 0),                        \
                    what ": misaligned labels or neighbour slice");                                                   \
        EMP_REQUIRE(top == 0 || top == 1, what ": top must be 0 or 1, got %d", top);                                  \
    } while (0)

static int64_t lm_rows(int64_t D, int64_t H, int top) { return D * H + (D + (top ? 1 : 0)) * (H + 1); }

extern "C" int64_t emp_label_mesh_count_work_bytes(int64_t R) { return emp_count_carve(nullptr, R).total; }

template <typename T, bool EMIT>
static int lm_launch(const void *lab, int64_t D, int64_t H, int64_t W, const void *below, const void *above, int top,
                     int64_t z_base, int32_t *row_counts, const int32_t *row_offsets, const LmOut &o, hipStream_t st)
{
    EMP_LAUNCH((lm_rows_kernel<T, EMIT>), emp_grid(lm_rows(D, H, top) * 64, 256, 16384), 256, st,
               reinterpret_cast<const T *>(lab), D, H, W, reinterpret_cast<const T *>(below),
               reinterpret_cast<const T *>(above), top, z_base, row_counts, row_offsets, o);
    return EMP_OK;
}

extern "C" int emp_label_mesh_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                    const void *above, int top, void *work, int64_t work_bytes, int32_t *row_offsets,
                                    void *stream)
{
    LM_REQUIRE_SHAPE("label_mesh_count");
    EMP_REQUIRE(work && row_offsets, "label_mesh_count: null pointer");
    const int64_t R = lm_rows(D, H, top);
    EmpCountWork L = emp_count_carve(work, R);
    EMP_REQUIRE(work_bytes >= L.total, "label_mesh_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    if (R == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, row_offsets, (int64_t)1);
        return EMP_OK;
    }
    const LmOut none = {};
    int rc = item == 4 ? lm_launch<uint32_t, false>(lab, D, H, W, below, above, top, 0, L.counts, nullptr, none, st)
                       : lm_launch<uint8_t, false>(lab, D, H, W, below, above, top, 0, L.counts, nullptr, none, st);
    if (rc != EMP_OK) return rc;
    return emp_exclusive_scan_i32(L.counts, R, row_offsets, L.scantmp, stream);
}

extern "C" int emp_label_mesh_emit(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                   const void *above, int top, int64_t z_base, const int32_t *row_offsets,
                                   int64_t n_quads, int64_t n_keys, uint64_t *vkeys, uint64_t *qkeys, int32_t *qdirs,
                                   void *stream)
{
    LM_REQUIRE_SHAPE("label_mesh_emit");
    EMP_REQUIRE(row_offsets, "label_mesh_emit: null pointer");
    EMP_REQUIRE(z_base >= 0 && z_base <= (1LL << 32) && (z_base + D + 1) <= (1LL << 32) / ((H + 1) * (W + 1)),
                "label_mesh_emit: (%lld + %lld + 1) x (%lld + 1) x (%lld + 1) corners exceed the limit of 2^32",
                (long long)z_base, (long long)D, (long long)H, (long long)W);
    EMP_REQUIRE(n_quads >= 0 && n_quads <= 6 * D * H * W && n_keys >= 0 && n_keys <= 8 * (D + 1) * (H + 1) * (W + 1),
                "label_mesh_emit: n_quads = %lld, n_keys = %lld are not the totals of this block", (long long)n_quads,
                (long long)n_keys);
    if (n_quads == 0 && n_keys == 0) return EMP_OK;
    EMP_REQUIRE((n_keys == 0 || vkeys) && (n_quads == 0 || (qkeys && qdirs)), "label_mesh_emit: null pointer");
    LmOut o;
    o.vkeys = vkeys;
    o.qkeys = qkeys;
    o.qdirs = qdirs;
    o.n_quads = n_quads;
    o.n_keys = n_keys;
    hipStream_t st = emp_stream(stream);
    return item == 4 ? lm_launch<uint32_t, true>(lab, D, H, W, below, above, top, z_base, nullptr, row_offsets, o, st)
                     : lm_launch<uint8_t, true>(lab, D, H, W, below, above, top, z_base, nullptr, row_offsets, o, st);
}

// ------------------------------------------------------------------------------------------ index
#define LM_OBJ_COLS 5

// Every sorted key becomes a vertex (z, y, x); the first key of a label opens the label's row of the objects table --
// label, v_begin, q_begin, q_end -- and closes the row before it (v_end).  Different rows, different slots: plain stores.
__global__ void lm_objects_kernel(const uint64_t *__restrict__ vkeys, int64_t nv, const int32_t *__restrict__ head,
                                  const int32_t *__restrict__ pos, const uint64_t *__restrict__ qkeys, int64_t nq,
                                  int64_t H, int64_t W, int32_t *__restrict__ vertices, int64_t *__restrict__ objects,
                                  int64_t max_objects)
{
    const uint64_t ey = (uint64_t)(W + 1), ez = (uint64_t)(H + 1) * ey;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = vkeys[i], corner = k & 0xffffffffULL;
        const uint64_t z = corner / ez, rem = corner - z * ez, y = rem / ey;
        vertices[3 * i] = (int32_t)z;
        vertices[3 * i + 1] = (int32_t)y;
        vertices[3 * i + 2] = (int32_t)(rem - y * ey);
        if (head[i]) {
            const int64_t row = pos[i];
            if (row < max_objects) {
                const uint64_t label = k >> 32;
                int64_t *o = objects + row * LM_OBJ_COLS;
                o[0] = (int64_t)label;
                o[1] = i;
                o[3] = emp_label_bound<false>(qkeys, 0, nq, label);
                o[4] = emp_label_bound<true>(qkeys, 0, nq, label);
            }
            if (row > 0 && row - 1 < max_objects) objects[(row - 1) * LM_OBJ_COLS + 2] = i;
        }
        if (i == nv - 1) {
            const int64_t last = (int64_t)pos[i] - (head[i] ? 0 : 1);
            if (last < max_objects) objects[last * LM_OBJ_COLS + 2] = nv;
        }
    }
}

// The four corners of quad i, in the winding of the header's table: o, o + a, o + a + b, o + b with (a, b) the two
// lattice steps of its direction; each is looked up among the keys of the quad's own object.  -1: no such vertex (the
// keys of a slab that does not own its top corner plane).
__global__ void lm_resolve_kernel(const uint64_t *__restrict__ qkeys, const int32_t *__restrict__ qdirs, int64_t nq,
                                  const uint64_t *__restrict__ vkeys, const int64_t *__restrict__ objects,
                                  const int32_t *__restrict__ n_objects, int64_t max_objects, int64_t H, int64_t W,
                                  int32_t *__restrict__ quads)
{
    const uint64_t ex = 1ull, ey = (uint64_t)(W + 1), ez = (uint64_t)(H + 1) * ey;
    int64_t n_obj = *n_objects;
    if (n_obj > max_objects) n_obj = max_objects;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = qkeys[i], label = k >> 32, o = k & 0xffffffffULL;
        const int d = qdirs[i];
        // -z: (ex, ey)  +z: (ey, ex)  -y: (ez, ex)  +y: (ex, ez)  -x: (ey, ez)  +x: (ez, ey)
        const uint64_t a = d == 0 ? ex : d == 1 ? ey : d == 2 ? ez : d == 3 ? ex : d == 4 ? ey : ez;
        const uint64_t b = d == 0 ? ey : d == 1 ? ex : d == 2 ? ex : d == 3 ? ez : d == 4 ? ez : ey;
        // the object's row: the last row whose label is <= this one
        int64_t lo = 0, hi = n_obj;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)objects[mid * LM_OBJ_COLS] < label) lo = mid + 1;
            else hi = mid;
        }
        int64_t vb = 0, ve = 0;
        if (lo < n_obj && (uint64_t)objects[lo * LM_OBJ_COLS] == label) {
            vb = objects[lo * LM_OBJ_COLS + 1];
            ve = objects[lo * LM_OBJ_COLS + 2];
        }
        const uint64_t c[4] = {o, o + a, o + a + b, o + b};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t want = (label << 32) | c[j];
            int64_t l = vb, h = ve;
            while (l < h) {
                const int64_t mid = l + ((h - l) >> 1);
                if (vkeys[mid] < want) l = mid + 1;
                else h = mid;
            }
            quads[4 * i + j] = (c[j] <= 0xffffffffULL && l < ve && vkeys[l] == want) ? (int32_t)l : -1;
        }
    }
}

struct LmIndexWork {
    int32_t *head, *pos, *scantmp;
    int64_t total;
};
static LmIndexWork lm_index_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    LmIndexWork L;
    L.head = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_label_mesh_index_work_bytes(int64_t nv) { return lm_index_carve(nullptr, nv).total; }

extern "C" int emp_label_mesh_index(const uint64_t *vkeys, int64_t nv, const uint64_t *qkeys, const int32_t *qdirs,
                                    int64_t nq, int64_t H, int64_t W, void *work, int64_t work_bytes, int32_t *vertices,
                                    int32_t *quads, int64_t *objects, int64_t max_objects, int32_t *n_objects,
                                    void *stream)
{
    EMP_REQUIRE(nv >= 0 && nv <= 0x7fffffffLL && nq >= 0 && nq <= 0x7fffffffLL,
                "label_mesh_index: %lld vertices, %lld quads: each must stay below 2^31", (long long)nv, (long long)nq);
    EMP_REQUIRE(H > 0 && W > 0 && (H + 1) <= (1LL << 32) / (W + 1), "label_mesh_index: bad shape (H = %lld, W = %lld)",
                (long long)H, (long long)W);
    EMP_REQUIRE(n_objects && max_objects >= 0, "label_mesh_index: null pointer");
    hipStream_t st = emp_stream(stream);
    if (nv == 0) {
        // no vertex: no quad can be resolved
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_objects, (int64_t)1);
        if (nq > 0) {
            EMP_REQUIRE(quads, "label_mesh_index: null pointer");
            if (hipMemsetAsync(quads, 0xff, (size_t)nq * 4 * sizeof(int32_t), st) != hipSuccess)
                EMP_FAIL(EMP_ELAUNCH, "label_mesh_index: memset failed");
        }
        return EMP_OK;
    }
    EMP_REQUIRE(vkeys && work && vertices && objects && (nq == 0 || (qkeys && qdirs && quads)),
                "label_mesh_index: null pointer");
    LmIndexWork L = lm_index_carve(work, nv);
    EMP_REQUIRE(work_bytes >= L.total, "label_mesh_index: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    const int grid = emp_grid(nv, 256, 4096);
    int rc = emp_compact(
        L.head, nv, L.pos, L.scantmp, n_objects, stream, "label_mesh_index: count copy",
        [&]() -> int {
            EMP_LAUNCH(emp_heads_kernel<32>, grid, 256, st, vkeys, nv, L.head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(lm_objects_kernel, grid, 256, st, vkeys, nv, L.head, L.pos, qkeys, nq, H, W, vertices, objects,
                       max_objects);
            return EMP_OK;
        });
    if (rc != EMP_OK) return rc;
    if (nq > 0)
        EMP_LAUNCH(lm_resolve_kernel, emp_grid(nq, 256, 4096), 256, st, qkeys, qdirs, nq, vkeys, objects, n_objects,
                   max_objects, H, W, quads);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ smoothing
__global__ void lm_fill_kernel(int32_t *__restrict__ v, int64_t n, int32_t value)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = value;
}

// Every quad edge joins two lattice neighbours: slot = 2 axis + (step > 0), the direction codes of the quads.  All the
// writers of a slot (the quads on both sides of the edge, up to four) write the same vertex: plain stores.
__global__ void lm_neighbours_kernel(const int32_t *__restrict__ vertices, int64_t nv, const int32_t *__restrict__ quads,
                                     int64_t nq, int32_t *__restrict__ nbr)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = quads[4 * i + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t a = q[j], b = q[(j + 1) & 3];
            if (a < 0 || b < 0 || a >= nv || b >= nv) continue;
            int slot = -1;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const int32_t d = vertices[3 * b + ax] - vertices[3 * a + ax];
                if (d != 0) slot = (slot == -1 && (d == 1 || d == -1)) ? 2 * ax + (d > 0 ? 1 : 0) : -2;
            }
            if (slot < 0) continue;                                             // not a lattice edge: not one of ours
            nbr[6 * a + slot] = (int32_t)b;
            nbr[6 * b + (slot ^ 1)] = (int32_t)a;
        }
    }
}

extern "C" int emp_mesh_neighbours(const int32_t *vertices, int64_t nv, const int32_t *quads, int64_t nq, int32_t *nbr,
                                   void *stream)
{
    EMP_REQUIRE(nv >= 0 && nv <= 0x7fffffffLL && nq >= 0 && nq <= 0x7fffffffLL,
                "mesh_neighbours: %lld vertices, %lld quads: each must stay below 2^31", (long long)nv, (long long)nq);
    if (nv == 0) return EMP_OK;
    EMP_REQUIRE(vertices && nbr && (nq == 0 || quads), "mesh_neighbours: null pointer");
    hipStream_t st = emp_stream(stream);
    EMP_LAUNCH(lm_fill_kernel, emp_grid(nv * 6, 256, 4096), 256, st, nbr, nv * 6, (int32_t)-1);
    if (nq > 0) EMP_LAUNCH(lm_neighbours_kernel, emp_grid(nq, 256, 4096), 256, st, vertices, nv, quads, nq, nbr);
    return EMP_OK;
}

// dst = src + factor (m - src), m the mean of the present neighbours added up in slot order; a vertex without a
// neighbour stays.  Gather only: src and dst are different arrays.
__global__ void lm_smooth_kernel(const float *__restrict__ src, const int32_t *__restrict__ nbr, int64_t nv, float factor,
                                 float *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        float s[3] = {0.f, 0.f, 0.f};
        int n = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int64_t j = nbr[6 * i + k];
            if (j >= 0 && j < nv) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) s[ax] += src[3 * j + ax];
                ++n;
            }
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float p = src[3 * i + ax];
            dst[3 * i + ax] = n ? p + factor * (s[ax] / (float)n - p) : p;
        }
    }
}

extern "C" int emp_mesh_smooth(const float *src, const int32_t *nbr, int64_t nv, float factor, float *dst, void *stream)
{
    EMP_REQUIRE(nv >= 0 && nv <= 0x7fffffffLL, "mesh_smooth: %lld vertices: must stay below 2^31", (long long)nv);
    if (nv == 0) return EMP_OK;
    EMP_REQUIRE(src && nbr && dst && src != dst, "mesh_smooth: null pointer, or src and dst are one array");
    EMP_LAUNCH(lm_smooth_kernel, emp_grid(nv, 256, 4096), 256, emp_stream(stream), src, nbr, nv, factor, dst);
    return EMP_OK;
}
