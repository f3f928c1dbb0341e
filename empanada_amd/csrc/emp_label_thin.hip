// Skeletons of the objects of a label volume (include/emp_hip.h, E8): topological thinning that keeps 1-D isthmuses,
// run by sub-fields, and the graph (vertices, edges, degrees) of a sparse label volume.  What users of the reference
// get on a CPU afterwards, object by object, from kimimaro or skimage.morphology.skeletonize; the definition is the
// header's.
//
// Predicate.  The 26 neighbours of a voxel that are alive and carry its label are one 26-bit mask M.  lt_classify
// floods bits over constant adjacency masks: c26 by growing the lowest set bit of M through LT_ADJ26 until nothing is
// added (M is one component iff the flood covers it), t6 by growing the lowest clear FACE position through LT_ADJ6
// inside the clear bits of the 18 face and edge positions (t6 = 1 iff the flood covers every clear face position).
// The adjacency masks are built by constexpr functions from the numbering itself, so no constant is typed by hand, and
// a flood takes at most a handful of rounds of a few bit operations: no table, no memory traffic.  The sweep and
// emp_skel_classify call this one function.
//
// State: one byte per voxel, bit 0 alive, bit 1 kept, bit 2 this iteration's mark.  A pass of sub-field s stores only
// bytes of voxels of sub-field s, and the decision for such a voxel reads only the alive bits of its 26 neighbours,
// none of which lies in s: a block may read a neighbour tile's bytes while that tile's block rewrites them.
//
// Tile: 8 x 8 x 64 voxels and 256 threads, as emp_label_grow.hip.  A pass stages alive ? label : 0 of the tile and its
// one-voxel ring in LDS (10 x 10 x 66 x 4 = 26 400 B: six blocks per CU by LDS on gfx950), then every thread examines
// two of the tile's 512 voxels of the sub-field.  Tiles start on even coordinates, so local and global parities agree in
// y and x; in z the caller's z_base decides.
//
// Due lists.  `pass` marks a tile as due for the passes: the mark step sets it when the tile holds an alive, marked,
// not-kept voxel, and a pass clears it when none is left.  `mark` marks a tile as due for the next mark step: the
// initialisation sets it for every listed tile, and a pass that deletes a voxel sets it for its own tile and for every
// tile whose ring holds that voxel -- behind faces, edges and corners, 26 directions.  A tile that is not due for the
// mark step keeps its marks: nothing in it or around it has changed, and a border voxel stays one while it lives.
// Nothing is atomic in global memory but the list's length in the initialisation and the counter of deleted voxels.
#include "emp_common.h"

#define LT_TZ EMP_TILE_Z
#define LT_TY EMP_TILE_Y
#define LT_TX EMP_TILE_X
#define LT_PZ (LT_TZ + 2)
#define LT_PY (LT_TY + 2)
#define LT_PX (LT_TX + 2)
#define LT_CELLS (LT_PZ * LT_PY * LT_PX)
#define LT_VOX (LT_TZ * LT_TY * LT_TX)
#define LT_THREADS 256
#define LT_ALIVE 1
#define LT_KEPT 2
#define LT_MARK 4
#define LT_MAX_VOXELS 0x7fffffffLL

typedef unsigned long long lt_u64;

// ------------------------------------------------------------------------------------------ the predicate
// the numbering of the 3 x 3 x 3 block (lt_pos, lt_dz, lt_dy, lt_dx) is emp_common.h's
static constexpr int lt_norm1(int n) { return lt_abs(lt_dz(n)) + lt_abs(lt_dy(n)) + lt_abs(lt_dx(n)); }
// the positions 26-adjacent to n: they differ from it by at most 1 in every coordinate
static constexpr uint32_t lt_adj26(int n)
{
    uint32_t m = 0;
    for (int k = 0; k < 26; ++k)
        if (k != n && lt_abs(lt_dz(k) - lt_dz(n)) <= 1 && lt_abs(lt_dy(k) - lt_dy(n)) <= 1 &&
            lt_abs(lt_dx(k) - lt_dx(n)) <= 1)
            m |= 1u << k;
    return m;
}
// among the 18 face and edge positions: those 6-adjacent to n
static constexpr uint32_t lt_adj6(int n)
{
    uint32_t m = 0;
    if (lt_norm1(n) > 2) return 0;
    for (int k = 0; k < 26; ++k)
        if (lt_norm1(k) <= 2 &&
            lt_abs(lt_dz(k) - lt_dz(n)) + lt_abs(lt_dy(k) - lt_dy(n)) + lt_abs(lt_dx(k) - lt_dx(n)) == 1)
            m |= 1u << k;
    return m;
}
static constexpr uint32_t lt_norm_mask(int most)
{
    uint32_t m = 0;
    for (int k = 0; k < 26; ++k)
        if (lt_norm1(k) <= most) m |= 1u << k;
    return m;
}
#define LT_ROW(f, a) f(a), f(a + 1), f(a + 2), f(a + 3), f(a + 4), f(a + 5), f(a + 6), f(a + 7), f(a + 8), f(a + 9), \
                     f(a + 10), f(a + 11), f(a + 12)
__device__ const uint32_t LT_ADJ26[26] = {LT_ROW(lt_adj26, 0), LT_ROW(lt_adj26, 13)};
__device__ const uint32_t LT_ADJ6[26] = {LT_ROW(lt_adj6, 0), LT_ROW(lt_adj6, 13)};
static constexpr uint32_t LT_FACE6 = lt_norm_mask(1), LT_FACE18 = lt_norm_mask(2);
static_assert(__builtin_popcount(LT_FACE6) == 6 && __builtin_popcount(LT_FACE18) == 18, "face and edge positions");
static_assert(__builtin_popcount(lt_adj26(0)) == 6 && __builtin_popcount(lt_adj26(4)) == 16, "26-adjacency");

// the part of `within` that `seed` reaches through adj
__device__ __forceinline__ uint32_t lt_flood(uint32_t seed, uint32_t within, const uint32_t *adj)
{
    uint32_t comp = seed, front = seed;
    while (front) {
        uint32_t next = 0;
        while (front) {
            next |= adj[__ffs((int)front) - 1];
            front &= front - 1;
        }
        front = next & within & ~comp;
        comp |= front;
    }
    return comp;
}

// bit 0: simple (c26 = 1 and t6 = 1), bit 1: isthmus (c26 >= 2)
__device__ __forceinline__ int lt_classify(uint32_t M)
{
    M &= 0x3ffffffu;
    if (M == 0) return 0;                                                       // c26 = 0: an isolated voxel stays
    if (lt_flood(M & (0u - M), M, LT_ADJ26) != M) return 2;
    const uint32_t B = ~M & LT_FACE18, F = B & LT_FACE6;
    if (F == 0) return 0;                                                       // t6 = 0: an interior voxel
    return (F & ~lt_flood(F & (0u - F), B, LT_ADJ6)) == 0 ? 1 : 0;
}

__global__ void lt_classify_kernel(const uint32_t *__restrict__ masks, int64_t n, uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)lt_classify(masks[i]);
}

extern "C" int emp_skel_classify(const uint32_t *masks, int64_t n, uint8_t *out, void *stream)
{
    EMP_REQUIRE(n >= 0 && n <= LT_MAX_VOXELS, "skel_classify: %lld masks outside 0 .. 2^31 - 1", (long long)n);
    if (n == 0) return EMP_OK;
    EMP_REQUIRE(masks && out, "skel_classify: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(masks) % 4) == 0, "skel_classify: misaligned pointer");
    EMP_LAUNCH(lt_classify_kernel, emp_grid(n, 256, 4096), 256, emp_stream(stream), masks, n, out);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ tiles and workspace
// counters[0]: length of the list; counters[1]: voxels deleted since the initialisation.  The layout is part of the
// interface (include/emp_hip.h, E8): tools read the due flags.
struct LtWork {
    lt_u64 *counters;
    int32_t *list;
    uint8_t *due_mark, *due_pass;
    int64_t total;
};
static LtWork lt_carve(void *work, int64_t n_tiles)
{
    if (n_tiles < 1) n_tiles = 1;
    EmpCarver c(work);
    LtWork L;
    L.counters = c.take<lt_u64>(2);
    L.list = c.take<int32_t>(n_tiles);
    L.due_mark = c.take<uint8_t>(n_tiles);
    L.due_pass = c.take<uint8_t>(n_tiles);
    L.total = c.bytes();
    return L;
}

extern "C" int64_t emp_label_thin_work_bytes(int64_t D, int64_t H, int64_t W)
{
    if (!emp_tiles_shape_ok(D, H, W)) return -1;
    return lt_carve(nullptr, emp_tiles(D, H, W).n).total;
}

#define LT_REQUIRE_SHAPE(what)                                                                                         \
    do {                                                                                                               \
        EMP_REQUIRE_VOLUME(what);                                                                                      \
        EMP_REQUIRE(emp_tiles_shape_ok(D, H, W),                                                                       \
                    what ": %lld x %lld x %lld voxels are more than 2^31 - 1; cut the slab into z-blocks",             \
                    (long long)D, (long long)H, (long long)W);                                                         \
    } while (0)

#define LT_REQUIRE_WORK(what)                                                                                          \
    const EmpTiles T = emp_tiles(D, H, W);                                                                             \
    LtWork L = lt_carve(work, T.n);                                                                                    \
    EMP_REQUIRE(work, what ": null pointer");                                                                          \
    EMP_REQUIRE(work_bytes >= L.total, what ": workspace too small (%lld < %lld)", (long long)work_bytes,              \
                (long long)L.total)

#define LT_REQUIRE_HALO(what)                                                                                          \
    do {                                                                                                               \
        EMP_REQUIRE((below_lab == nullptr) == (below_state == nullptr) &&                                              \
                        (above_lab == nullptr) == (above_state == nullptr),                                            \
                    what ": a halo is one slice of labels AND one of state, or neither");                              \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 &&                                       \
                        (reinterpret_cast<uintptr_t>(below_lab) % (uintptr_t)item) == 0 &&                             \
                        (reinterpret_cast<uintptr_t>(above_lab) % (uintptr_t)item) == 0,                               \
                    what ": misaligned pointer");                                                                      \
    } while (0)

__global__ void lt_clear_kernel(int64_t n_tiles, lt_u64 *__restrict__ counters, uint8_t *__restrict__ due_mark,
                                uint8_t *__restrict__ due_pass)
{
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 < 2) counters[i0] = 0;
    for (int64_t i = i0; i < n_tiles; i += (int64_t)gridDim.x * blockDim.x) due_mark[i] = due_pass[i] = 0;
}

// ------------------------------------------------------------------------------------------ init
template <typename T>
__global__ __launch_bounds__(LT_THREADS) void lt_init_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                             EmpTiles tiles, uint8_t *__restrict__ state,
                                                             lt_u64 *counters, int32_t *__restrict__ list,
                                                             uint8_t *__restrict__ due_mark)
{
    for (int64_t tile = blockIdx.x; tile < tiles.n; tile += gridDim.x) {
        const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
        int any = 0;
        for (int i = threadIdx.x; i < LT_VOX; i += LT_THREADS) {
            const int lx = i & (LT_TX - 1), ly = (i / LT_TX) & (LT_TY - 1), lz = i / (LT_TX * LT_TY);
            const int64_t z = tz * LT_TZ + lz, y = ty * LT_TY + ly, x = tx * LT_TX + lx;
            if (z >= D || y >= H || x >= W) continue;
            const int64_t at = (z * H + y) * W + x;
            const int alive = lab[at] != 0 ? LT_ALIVE : 0;
            state[at] = (uint8_t)alive;
            any |= alive;
        }
        any = __syncthreads_or(any);
        if (threadIdx.x == 0 && any) {
            list[atomicAdd(counters, 1ULL)] = (int32_t)tile;
            due_mark[tile] = 1;
        }
    }
}

extern "C" int emp_label_thin_init(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint8_t *state,
                                   void *work, int64_t work_bytes, void *stream)
{
    LT_REQUIRE_SHAPE("label_thin_init");
    if (D == 0) return EMP_OK;
    LT_REQUIRE_WORK("label_thin_init");
    EMP_REQUIRE(lab && state, "label_thin_init: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0, "label_thin_init: misaligned pointer");
    hipStream_t st = emp_stream(stream);
    EMP_LAUNCH(lt_clear_kernel, emp_grid(T.n > 16 ? T.n : 16, 256, 1024), 256, st, T.n, L.counters, L.due_mark,
               L.due_pass);
    const int grid = emp_grid(T.n, 1, 16384);
    if (item == 4)
        EMP_LAUNCH((lt_init_kernel<uint32_t>), grid, LT_THREADS, st, reinterpret_cast<const uint32_t *>(lab), D, H, W, T,
                   state, L.counters, L.list, L.due_mark);
    else
        EMP_LAUNCH((lt_init_kernel<uint8_t>), grid, LT_THREADS, st, reinterpret_cast<const uint8_t *>(lab), D, H, W, T,
                   state, L.counters, L.list, L.due_mark);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ mark and pass
template <typename T>
struct LtHalo {
    const T *lab_below, *lab_above;          // one (H, W) slice each, null = the volume's face
    const uint8_t *st_below, *st_above;
};

__device__ __forceinline__ uint8_t lt_peek(const uint8_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// alive ? label : 0 of position (z, y, x), z in -1 .. D; everything outside the volume and its two halo slices is 0
template <typename T>
__device__ __forceinline__ uint32_t lt_object(const T *__restrict__ lab, const uint8_t *state, const LtHalo<T> &halo,
                                              int64_t D, int64_t H, int64_t W, int64_t z, int64_t y, int64_t x)
{
    if (y < 0 || y >= H || x < 0 || x >= W) return 0;
    if (z >= 0 && z < D) {
        const int64_t at = (z * H + y) * W + x;
        return (lt_peek(state + at) & LT_ALIVE) ? (uint32_t)lab[at] : 0u;
    }
    if (z == -1 && halo.lab_below) return (lt_peek(halo.st_below + y * W + x) & LT_ALIVE) ? (uint32_t)halo.lab_below[y * W + x] : 0u;
    if (z == D && halo.lab_above) return (lt_peek(halo.st_above + y * W + x) & LT_ALIVE) ? (uint32_t)halo.lab_above[y * W + x] : 0u;
    return 0;
}

// Step 1: every alive voxel of a due tile with a face neighbour outside its object is marked; the tile is due for the
// passes iff it then holds an alive, marked, not-kept voxel.  Only bit 2 of the tile's own bytes changes.
template <typename T>
__global__ __launch_bounds__(LT_THREADS) void lt_mark_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                             EmpTiles tiles, LtHalo<T> halo, uint8_t *state,
                                                             const int32_t *__restrict__ list, uint8_t *due_mark,
                                                             uint8_t *due_pass, int force)
{
    const int64_t tile = list[blockIdx.x];
    const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
    const bool run = due_mark[tile] || ((force & 1) && tz == 0) || ((force & 2) && tz + 1 == tiles.nz);
    __syncthreads();                              // every thread has read the flag before it is taken back
    if (!run) return;
    if (threadIdx.x == 0) due_mark[tile] = 0;
    int cand = 0;
    for (int i = threadIdx.x; i < LT_VOX; i += LT_THREADS) {
        const int lx = i & (LT_TX - 1), ly = (i / LT_TX) & (LT_TY - 1), lz = i / (LT_TX * LT_TY);
        const int64_t z = tz * LT_TZ + lz, y = ty * LT_TY + ly, x = tx * LT_TX + lx;
        if (z >= D || y >= H || x >= W) continue;
        const int64_t at = (z * H + y) * W + x;
        const uint8_t old = state[at];
        uint8_t now = old & (LT_ALIVE | LT_KEPT);
        if (old & LT_ALIVE) {
            const uint32_t l = (uint32_t)lab[at];
            const bool inside = lt_object(lab, state, halo, D, H, W, z - 1, y, x) == l &&
                                lt_object(lab, state, halo, D, H, W, z + 1, y, x) == l &&
                                lt_object(lab, state, halo, D, H, W, z, y - 1, x) == l &&
                                lt_object(lab, state, halo, D, H, W, z, y + 1, x) == l &&
                                lt_object(lab, state, halo, D, H, W, z, y, x - 1) == l &&
                                lt_object(lab, state, halo, D, H, W, z, y, x + 1) == l;
            if (!inside) now |= LT_MARK;
        }
        if (now != old) state[at] = now;
        cand |= (now & (LT_ALIVE | LT_KEPT | LT_MARK)) == (LT_ALIVE | LT_MARK);
    }
    cand = __syncthreads_or(cand);
    if (threadIdx.x == 0) due_pass[tile] = cand ? 1 : 0;
}

// Step 2 for one sub-field.  pz: the parity of the LOCAL z of the sub-field's voxels (the caller folds z_base in).
template <typename T>
__global__ __launch_bounds__(LT_THREADS) void lt_pass_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                             EmpTiles tiles, LtHalo<T> halo, uint8_t *state,
                                                             const int32_t *__restrict__ list, uint8_t *due_mark,
                                                             uint8_t *due_pass, int pz, int py, int px,
                                                             lt_u64 *counter)
{
    __shared__ uint32_t s_obj[LT_CELLS];
    __shared__ unsigned s_dirs;
    __shared__ int s_cand, s_done, s_deleted;
    const int64_t tile = list[blockIdx.x];
    if (!due_pass[tile]) return;
    const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
    const int64_t z0 = tz * LT_TZ - 1, y0 = ty * LT_TY - 1, x0 = tx * LT_TX - 1;
    if (threadIdx.x == 0) {
        s_dirs = 0;
        s_cand = s_done = s_deleted = 0;
    }
    __syncthreads();
    // 1. alive ? label : 0 of the tile and its ring; the tile's own voxels that are still to be decided are counted
    int cand = 0;
    for (int c = threadIdx.x; c < LT_CELLS; c += LT_THREADS) {
        const int lx = c % LT_PX, ly = (c / LT_PX) % LT_PY, lz = c / (LT_PX * LT_PY);
        const int64_t z = z0 + lz, y = y0 + ly, x = x0 + lx;
        s_obj[c] = lt_object(lab, state, halo, D, H, W, z, y, x);
        if (lz >= 1 && lz <= LT_TZ && ly >= 1 && ly <= LT_TY && lx >= 1 && lx <= LT_TX && z < D && y < H && x < W)
            cand += (state[(z * H + y) * W + x] & (LT_ALIVE | LT_KEPT | LT_MARK)) == (LT_ALIVE | LT_MARK);
    }
    if (cand) atomicAdd(&s_cand, cand);
    __syncthreads();
    // 2. the sub-field's 4 x 4 x 32 voxels of the tile, two per thread
    int done = 0, deleted = 0;
    unsigned dirs = 0;
    for (int k = 0; k < LT_VOX / 8 / LT_THREADS; ++k) {
        const int j = threadIdx.x + k * LT_THREADS;
        const int lx = 2 * (j & (LT_TX / 2 - 1)) + px, ly = 2 * ((j / (LT_TX / 2)) & (LT_TY / 2 - 1)) + py,
                  lz = 2 * (j / (LT_TX / 2 * (LT_TY / 2))) + pz;
        const int64_t z = z0 + 1 + lz, y = y0 + 1 + ly, x = x0 + 1 + lx;
        if (z >= D || y >= H || x >= W) continue;
        const int64_t at = (z * H + y) * W + x;
        const uint8_t st = state[at];
        if ((st & (LT_ALIVE | LT_KEPT | LT_MARK)) != (LT_ALIVE | LT_MARK)) continue;
        const int c = ((lz + 1) * LT_PY + ly + 1) * LT_PX + lx + 1;
        const uint32_t l = s_obj[c];
        uint32_t M = 0;
#pragma unroll
        for (int n = 0; n < 26; ++n)
            M |= (s_obj[c + (lt_dz(n) * LT_PY + lt_dy(n)) * LT_PX + lt_dx(n)] == l ? 1u : 0u) << n;
        const int cls = lt_classify(M);
        if (cls & 2) {
            state[at] = st | LT_KEPT;
            ++done;
        } else if (cls & 1) {
            state[at] = 0;
            ++done;
            ++deleted;
            // the tiles whose ring holds this voxel (and the tile itself): 27 directions, bit 9 (dz+1) + 3 (dy+1) + dx+1
            for (int dz = (lz == 0 ? -1 : 0); dz <= (lz == LT_TZ - 1 ? 1 : 0); ++dz)
                for (int dy = (ly == 0 ? -1 : 0); dy <= (ly == LT_TY - 1 ? 1 : 0); ++dy)
                    for (int dx = (lx == 0 ? -1 : 0); dx <= (lx == LT_TX - 1 ? 1 : 0); ++dx)
                        dirs |= 1u << (9 * (dz + 1) + 3 * (dy + 1) + dx + 1);
        }
    }
    if (done) atomicAdd(&s_done, done);
    if (deleted) atomicAdd(&s_deleted, deleted);
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();
    // 3. the report: the counter, the tile's own flag, and the tiles that have to be marked anew
    if (threadIdx.x == 0) {
        if (s_deleted) atomicAdd(counter, (lt_u64)s_deleted);
        if (s_cand == s_done) due_pass[tile] = 0;
    }
    if (threadIdx.x < 27 && ((s_dirs >> threadIdx.x) & 1u)) {
        const int dz = (int)threadIdx.x / 9 - 1, dy = ((int)threadIdx.x / 3) % 3 - 1, dx = (int)threadIdx.x % 3 - 1;
        const int64_t nz = tz + dz, ny = ty + dy, nx = tx + dx;
        if (nz >= 0 && nz < tiles.nz && ny >= 0 && ny < tiles.ny && nx >= 0 && nx < tiles.nx)
            due_mark[(nz * tiles.ny + ny) * tiles.nx + nx] = 1;
    }
}

#define LT_SWEEP_ARGS                                                                                                  \
    const void *lab, int item, int64_t D, int64_t H, int64_t W, uint8_t *state, const void *below_lab,                 \
        const uint8_t *below_state, const void *above_lab, const uint8_t *above_state, void *work, int64_t work_bytes, \
        int64_t n_listed

extern "C" int emp_label_thin_mark(LT_SWEEP_ARGS, int force, void *stream)
{
    LT_REQUIRE_SHAPE("label_thin_mark");
    LT_REQUIRE_HALO("label_thin_mark");
    EMP_REQUIRE(force >= 0 && force <= 3, "label_thin_mark: force = %d outside 0 .. 3", force);
    EMP_REQUIRE(n_listed >= 0 && n_listed <= emp_tiles(D, H, W).n, "label_thin_mark: %lld listed tiles, the slab has %lld",
                (long long)n_listed, (long long)emp_tiles(D, H, W).n);
    if (D == 0 || n_listed == 0) return EMP_OK;
    EMP_REQUIRE(lab && state, "label_thin_mark: null pointer");
    LT_REQUIRE_WORK("label_thin_mark");
    hipStream_t st = emp_stream(stream);
    if (item == 4) {
        LtHalo<uint32_t> halo = {reinterpret_cast<const uint32_t *>(below_lab), reinterpret_cast<const uint32_t *>(above_lab),
                                 below_state, above_state};
        EMP_LAUNCH((lt_mark_kernel<uint32_t>), (int)n_listed, LT_THREADS, st, reinterpret_cast<const uint32_t *>(lab), D, H,
                   W, T, halo, state, L.list, L.due_mark, L.due_pass, force);
    } else {
        LtHalo<uint8_t> halo = {reinterpret_cast<const uint8_t *>(below_lab), reinterpret_cast<const uint8_t *>(above_lab),
                                below_state, above_state};
        EMP_LAUNCH((lt_mark_kernel<uint8_t>), (int)n_listed, LT_THREADS, st, reinterpret_cast<const uint8_t *>(lab), D, H, W,
                   T, halo, state, L.list, L.due_mark, L.due_pass, force);
    }
    return EMP_OK;
}

extern "C" int emp_label_thin_pass(LT_SWEEP_ARGS, int subfield, int64_t z_base, void *stream)
{
    LT_REQUIRE_SHAPE("label_thin_pass");
    LT_REQUIRE_HALO("label_thin_pass");
    EMP_REQUIRE(subfield >= 0 && subfield <= 7, "label_thin_pass: subfield = %d outside 0 .. 7", subfield);
    EMP_REQUIRE(z_base >= 0, "label_thin_pass: z_base = %lld is negative", (long long)z_base);
    EMP_REQUIRE(n_listed >= 0 && n_listed <= emp_tiles(D, H, W).n, "label_thin_pass: %lld listed tiles, the slab has %lld",
                (long long)n_listed, (long long)emp_tiles(D, H, W).n);
    if (D == 0 || n_listed == 0) return EMP_OK;
    EMP_REQUIRE(lab && state, "label_thin_pass: null pointer");
    LT_REQUIRE_WORK("label_thin_pass");
    hipStream_t st = emp_stream(stream);
    const int pz = ((subfield >> 2) ^ (int)(z_base & 1)) & 1, py = (subfield >> 1) & 1, px = subfield & 1;
    if (item == 4) {
        LtHalo<uint32_t> halo = {reinterpret_cast<const uint32_t *>(below_lab), reinterpret_cast<const uint32_t *>(above_lab),
                                 below_state, above_state};
        EMP_LAUNCH((lt_pass_kernel<uint32_t>), (int)n_listed, LT_THREADS, st, reinterpret_cast<const uint32_t *>(lab), D, H,
                   W, T, halo, state, L.list, L.due_mark, L.due_pass, pz, py, px, L.counters + 1);
    } else {
        LtHalo<uint8_t> halo = {reinterpret_cast<const uint8_t *>(below_lab), reinterpret_cast<const uint8_t *>(above_lab),
                                below_state, above_state};
        EMP_LAUNCH((lt_pass_kernel<uint8_t>), (int)n_listed, LT_THREADS, st, reinterpret_cast<const uint8_t *>(lab), D, H, W,
                   T, halo, state, L.list, L.due_mark, L.due_pass, pz, py, px, L.counters + 1);
    }
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ paint
template <typename T, typename O>
__global__ void lt_paint_kernel(int64_t n, const uint8_t *__restrict__ state, const T *lab, O *dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (state[i] & LT_ALIVE) ? (O)lab[i] : (O)0;
}

extern "C" int emp_label_thin_paint(const uint8_t *state, const void *lab, int item, int64_t n, void *dst, int dst_item,
                                    void *stream)
{
    EMP_REQUIRE(item == 1 || item == 4, "label_thin_paint: labels must be uint8 (1) or uint32 (4), got %d bytes", item);
    EMP_REQUIRE(dst_item == 1 || dst_item == 4, "label_thin_paint: dst must be uint8 (1) or uint32 (4), got %d bytes",
                dst_item);
    EMP_REQUIRE(n >= 0 && n <= LT_MAX_VOXELS, "label_thin_paint: %lld voxels outside 0 .. 2^31 - 1", (long long)n);
    if (n == 0) return EMP_OK;
    EMP_REQUIRE(state && lab && dst, "label_thin_paint: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 &&
                    (reinterpret_cast<uintptr_t>(dst) % (uintptr_t)dst_item) == 0,
                "label_thin_paint: misaligned pointer");
    const char *l0 = reinterpret_cast<const char *>(lab), *l1 = l0 + n * item;
    const char *d0 = reinterpret_cast<const char *>(dst), *d1 = d0 + n * dst_item;
    const char *s0 = reinterpret_cast<const char *>(state), *s1 = s0 + n;
    EMP_REQUIRE((d0 == l0 && dst_item == item) || d1 <= l0 || d0 >= l1,
                "label_thin_paint: dst overlaps the labels without being the labels themselves");
    EMP_REQUIRE(d1 <= s0 || d0 >= s1, "label_thin_paint: dst overlaps the state");
    hipStream_t st = emp_stream(stream);
    const int grid = emp_grid(n, 256, 16384);
    if (item == 4 && dst_item == 4)
        EMP_LAUNCH((lt_paint_kernel<uint32_t, uint32_t>), grid, 256, st, n, state, reinterpret_cast<const uint32_t *>(lab),
                   reinterpret_cast<uint32_t *>(dst));
    else if (item == 4)
        EMP_LAUNCH((lt_paint_kernel<uint32_t, uint8_t>), grid, 256, st, n, state, reinterpret_cast<const uint32_t *>(lab),
                   reinterpret_cast<uint8_t *>(dst));
    else if (dst_item == 4)
        EMP_LAUNCH((lt_paint_kernel<uint8_t, uint32_t>), grid, 256, st, n, state, reinterpret_cast<const uint8_t *>(lab),
                   reinterpret_cast<uint32_t *>(dst));
    else
        EMP_LAUNCH((lt_paint_kernel<uint8_t, uint8_t>), grid, 256, st, n, state, reinterpret_cast<const uint8_t *>(lab),
                   reinterpret_cast<uint8_t *>(dst));
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ graph: count and emit
// One wave per row (z, y), 64 voxels at a time; a chunk of background alone is left at once.  A voxel with S != 0 is a
// vertex; it owns the edges to its same-label neighbours at the 13 offsets above (0, 0, 0) -- bits 13 .. 25 of its
// neighbourhood mask -- and its degree is the mask's population.  Positions are prefix sums: rows 0 .. R - 1 of
// row_offsets count vertices, rows R .. 2 R - 1 edges.
#define LG2_MAX_VOXELS (1LL << 26)            // 1 vertex and 13 edges per voxel at most: the int32 scan stays exact

struct LtGraphOut {
    uint64_t *vkeys;    // label << 32 | global voxel number, in voxel order
    int32_t *vdeg;      // the vertex's degree
    uint64_t *ekeys;    // label << 32 | the edge's lower voxel, in (voxel, code) order
    int32_t *ecodes;    // 0 .. 12: the offset to the upper voxel
    int64_t nv, ne;
};

template <typename T, bool EMIT>
__global__ __launch_bounds__(256) void lt_graph_rows_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                            const T *__restrict__ below, const T *__restrict__ above,
                                                            int64_t z_base, int32_t *__restrict__ row_counts,
                                                            const int32_t *__restrict__ row_offsets, LtGraphOut o)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t R = D * H;
    for (int64_t row = wave; row < R; row += n_waves) {
        const int64_t z = row / H, y = row - z * H;
        const T *src = lab + row * W;
        const int64_t vbase = EMIT ? (int64_t)row_offsets[row] : 0;
        const int64_t ebase = EMIT ? (int64_t)row_offsets[R + row] - (int64_t)row_offsets[R] : 0;
        int run_v = 0, run_e = 0;                                               // wave uniform
        for (int64_t x0 = 0; x0 < W; x0 += 64) {
            const int64_t x = x0 + lane;
            const uint32_t l = x < W ? (uint32_t)src[x] : 0u;
            const lt_u64 present = __ballot(l != 0u);
            if (present == 0ull) continue;
            uint32_t M = 0;
            if (l != 0u) {
#pragma unroll
                for (int n = 0; n < 26; ++n)
                    M |= (lt_label_at<T>(lab, below, above, D, H, W, z + lt_dz(n), y + lt_dy(n), x + lt_dx(n)) == l ? 1u : 0u)
                         << n;
            }
            const uint32_t upper = M >> 13;
            const int ne = __popc(upper);
            int incl = ne;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (EMIT && l != 0u) {
                const uint64_t voxel = (uint64_t)((z_base + z) * H + y) * (uint64_t)W + (uint64_t)x;
                const int64_t pv = vbase + run_v + __popcll(present & ((1ull << lane) - 1ull));
                if (pv < o.nv) {
                    o.vkeys[pv] = ((uint64_t)l << 32) | voxel;
                    o.vdeg[pv] = __popc(M);
                }
                int64_t pe = ebase + run_e + (incl - ne);
#pragma unroll
                for (int c = 0; c < 13; ++c) {
                    if ((upper >> c) & 1u) {
                        if (pe < o.ne) {
                            o.ekeys[pe] = ((uint64_t)l << 32) | voxel;
                            o.ecodes[pe] = c;
                        }
                        ++pe;
                    }
                }
            }
            run_v += __popcll(present);
            run_e += __shfl(incl, 63);
        }
        if (!EMIT && lane == 0) {
            row_counts[row] = run_v;
            row_counts[R + row] = run_e;
        }
    }
}

#define LG2_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                              \
        EMP_REQUIRE_VOLUME(what);                                                                                     \
        EMP_REQUIRE(H <= LG2_MAX_VOXELS / W && (D == 0 || H * W <= LG2_MAX_VOXELS / D),                               \
                    what ": %lld x %lld x %lld voxels exceed 2^26 per call; cut the slab into z-blocks",              \
                    (long long)D, (long long)H, (long long)W);                                                        \
        EMP_REQUIRE(D == 0 || lab, what ": null pointer");                                                            \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 &&                                      \
                        (reinterpret_cast<uintptr_t>(below) % (uintptr_t)item) == 0 &&                                \
                        (reinterpret_cast<uintptr_t>(above) % (uintptr_t)item) == 0,                                  \
                    what ": misaligned labels or neighbour slice");                                                   \
    } while (0)

extern "C" int64_t emp_label_graph_count_work_bytes(int64_t R) { return R < 0 ? -1 : emp_count_carve(nullptr, 2 * R).total; }

template <typename T, bool EMIT>
static int lt_graph_launch(const void *lab, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                           int64_t z_base, int32_t *row_counts, const int32_t *row_offsets, const LtGraphOut &o,
                           hipStream_t st)
{
    EMP_LAUNCH((lt_graph_rows_kernel<T, EMIT>), emp_grid(D * H * 64, 256, 16384), 256, st,
               reinterpret_cast<const T *>(lab), D, H, W, reinterpret_cast<const T *>(below),
               reinterpret_cast<const T *>(above), z_base, row_counts, row_offsets, o);
    return EMP_OK;
}

extern "C" int emp_label_graph_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                     const void *above, void *work, int64_t work_bytes, int32_t *row_offsets,
                                     void *stream)
{
    LG2_REQUIRE_SHAPE("label_graph_count");
    EMP_REQUIRE(work && row_offsets, "label_graph_count: null pointer");
    const int64_t R = D * H;
    EmpCountWork L = emp_count_carve(work, 2 * R);
    EMP_REQUIRE(work_bytes >= L.total, "label_graph_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    if (R == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, row_offsets, (int64_t)1);
        return EMP_OK;
    }
    const LtGraphOut none = {};
    int rc = item == 4 ? lt_graph_launch<uint32_t, false>(lab, D, H, W, below, above, 0, L.counts, nullptr, none, st)
                       : lt_graph_launch<uint8_t, false>(lab, D, H, W, below, above, 0, L.counts, nullptr, none, st);
    if (rc != EMP_OK) return rc;
    return emp_exclusive_scan_i32(L.counts, 2 * R, row_offsets, L.scantmp, stream);
}

extern "C" int emp_label_graph_emit(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                    const void *above, int64_t z_base, const int32_t *row_offsets, int64_t nv,
                                    int64_t ne, uint64_t *vkeys, int32_t *vdeg, uint64_t *ekeys, int32_t *ecodes,
                                    void *stream)
{
    LG2_REQUIRE_SHAPE("label_graph_emit");
    EMP_REQUIRE(row_offsets, "label_graph_emit: null pointer");
    EMP_REQUIRE(z_base >= 0 && z_base <= (1LL << 32) && (z_base + D) <= (1LL << 32) / (H * W),
                "label_graph_emit: (%lld + %lld) x %lld x %lld voxels exceed the limit of 2^32", (long long)z_base,
                (long long)D, (long long)H, (long long)W);
    EMP_REQUIRE(nv >= 0 && nv <= D * H * W && ne >= 0 && ne <= 13 * D * H * W,
                "label_graph_emit: nv = %lld, ne = %lld are not the totals of this block", (long long)nv, (long long)ne);
    if (nv == 0 && ne == 0) return EMP_OK;
    EMP_REQUIRE((nv == 0 || (vkeys && vdeg)) && (ne == 0 || (ekeys && ecodes)), "label_graph_emit: null pointer");
    LtGraphOut o;
    o.vkeys = vkeys;
    o.vdeg = vdeg;
    o.ekeys = ekeys;
    o.ecodes = ecodes;
    o.nv = nv;
    o.ne = ne;
    hipStream_t st = emp_stream(stream);
    return item == 4 ? lt_graph_launch<uint32_t, true>(lab, D, H, W, below, above, z_base, nullptr, row_offsets, o, st)
                     : lt_graph_launch<uint8_t, true>(lab, D, H, W, below, above, z_base, nullptr, row_offsets, o, st);
}

// ------------------------------------------------------------------------------------------ graph: index
#define LG2_OBJ_COLS 8

// head = the first key of a label; iso / end / junc = the vertex has degree 0 / 1 / >= 3
__global__ void lt_flags_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ deg, int64_t n,
                                int32_t *__restrict__ head, int32_t *__restrict__ iso, int32_t *__restrict__ end,
                                int32_t *__restrict__ junc)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        head[i] = (i == 0 || (keys[i - 1] >> 32) != (keys[i] >> 32)) ? 1 : 0;
        const int d = deg[i];
        iso[i] = d == 0;
        end[i] = d == 1;
        junc[i] = d >= 3;
    }
}

// Every sorted key becomes a vertex (z, y, x); the first key of a label opens the label's row of the objects table and
// closes the row before it.  Different rows, different slots: plain stores.
__global__ void lt_objects_kernel(const uint64_t *__restrict__ vkeys, int64_t nv, const int32_t *__restrict__ head,
                                  const int32_t *__restrict__ pos, const uint64_t *__restrict__ ekeys, int64_t ne,
                                  int64_t H, int64_t W, int32_t *__restrict__ vertices, int64_t *__restrict__ objects,
                                  int64_t max_objects)
{
    const uint64_t ey = (uint64_t)W, ez = (uint64_t)H * ey;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = vkeys[i], voxel = k & 0xffffffffULL;
        const uint64_t z = voxel / ez, rem = voxel - z * ez, y = rem / ey;
        vertices[3 * i] = (int32_t)z;
        vertices[3 * i + 1] = (int32_t)y;
        vertices[3 * i + 2] = (int32_t)(rem - y * ey);
        if (head[i]) {
            const int64_t row = pos[i];
            if (row < max_objects) {
                const uint64_t label = k >> 32;
                int64_t *o = objects + row * LG2_OBJ_COLS;
                o[0] = (int64_t)label;
                o[1] = i;
                o[3] = emp_label_bound<false>(ekeys, 0, ne, label);
                o[4] = emp_label_bound<true>(ekeys, 0, ne, label);
            }
            if (row > 0 && row - 1 < max_objects) objects[(row - 1) * LG2_OBJ_COLS + 2] = i;
        }
        if (i == nv - 1) {
            const int64_t last = (int64_t)pos[i] - (head[i] ? 0 : 1);
            if (last < max_objects) objects[last * LG2_OBJ_COLS + 2] = nv;
        }
    }
}

// columns 5 .. 7 of an object: differences of the three prefix sums over its [v_begin, v_end)
__global__ void lt_object_counts_kernel(const int32_t *__restrict__ n_objects, int64_t max_objects,
                                        const int32_t *__restrict__ p_iso, const int32_t *__restrict__ p_end,
                                        const int32_t *__restrict__ p_junc, int64_t *__restrict__ objects)
{
    int64_t n = *n_objects;
    if (n > max_objects) n = max_objects;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t *o = objects + r * LG2_OBJ_COLS;
        const int64_t b = o[1], e = o[2];
        o[5] = p_iso[e] - p_iso[b];
        o[6] = p_end[e] - p_end[b];
        o[7] = p_junc[e] - p_junc[b];
    }
}

// Edge i joins its lower voxel u and u + the offset of its code; both are looked up among the keys of the edge's own
// object.  -1: no such vertex (keys that are not a whole volume's).
__global__ void lt_edges_kernel(const uint64_t *__restrict__ ekeys, const int32_t *__restrict__ ecodes, int64_t ne,
                                const uint64_t *__restrict__ vkeys, const int64_t *__restrict__ objects,
                                const int32_t *__restrict__ n_objects, int64_t max_objects, int64_t H, int64_t W,
                                int32_t *__restrict__ edges)
{
    int64_t n_obj = *n_objects;
    if (n_obj > max_objects) n_obj = max_objects;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = ekeys[i], label = k >> 32;
        const int64_t u = (int64_t)(k & 0xffffffffULL);
        const int p = 14 + ecodes[i];                                           // position in the 3 x 3 x 3 block
        const int64_t w = u + (int64_t)(p / 9 - 1) * H * W + (int64_t)((p / 3) % 3 - 1) * W + (p % 3 - 1);
        int64_t lo = 0, hi = n_obj;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)objects[mid * LG2_OBJ_COLS] < label) lo = mid + 1;
            else hi = mid;
        }
        int64_t vb = 0, ve = 0;
        if (lo < n_obj && (uint64_t)objects[lo * LG2_OBJ_COLS] == label) {
            vb = objects[lo * LG2_OBJ_COLS + 1];
            ve = objects[lo * LG2_OBJ_COLS + 2];
        }
        const int64_t end[2] = {u, w};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint64_t want = (label << 32) | (uint64_t)end[j];
            int64_t l = vb, h = ve;
            while (l < h) {
                const int64_t mid = l + ((h - l) >> 1);
                if (vkeys[mid] < want) l = mid + 1;
                else h = mid;
            }
            edges[2 * i + j] = (end[j] >= 0 && end[j] <= 0xffffffffLL && l < ve && vkeys[l] == want) ? (int32_t)l : -1;
        }
    }
}

struct LtIndexWork {
    int32_t *head, *iso, *end, *junc, *pos, *p_iso, *p_end, *p_junc, *scantmp;
    int64_t total;
};
static LtIndexWork lt_index_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    LtIndexWork L;
    L.head = c.take<int32_t>(n);
    L.iso = c.take<int32_t>(n);
    L.end = c.take<int32_t>(n);
    L.junc = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.p_iso = c.take<int32_t>(n + 1);
    L.p_end = c.take<int32_t>(n + 1);
    L.p_junc = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_label_graph_index_work_bytes(int64_t nv) { return nv < 0 ? -1 : lt_index_carve(nullptr, nv).total; }

extern "C" int emp_label_graph_index(const uint64_t *vkeys, const int32_t *vdeg, int64_t nv, const uint64_t *ekeys,
                                     const int32_t *ecodes, int64_t ne, int64_t H, int64_t W, void *work,
                                     int64_t work_bytes, int32_t *vertices, int32_t *edges, int64_t *objects,
                                     int64_t max_objects, int32_t *n_objects, void *stream)
{
    EMP_REQUIRE(nv >= 0 && nv <= 0x7fffffffLL && ne >= 0 && ne <= 0x7fffffffLL,
                "label_graph_index: %lld vertices, %lld edges: each must stay below 2^31", (long long)nv, (long long)ne);
    EMP_REQUIRE(H > 0 && W > 0 && H <= (1LL << 32) / W, "label_graph_index: bad shape (H = %lld, W = %lld)",
                (long long)H, (long long)W);
    EMP_REQUIRE(n_objects && max_objects >= 0, "label_graph_index: null pointer");
    hipStream_t st = emp_stream(stream);
    if (nv == 0) {
        // no vertex: no edge can be resolved
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_objects, (int64_t)1);
        if (ne > 0) {
            EMP_REQUIRE(edges, "label_graph_index: null pointer");
            if (hipMemsetAsync(edges, 0xff, (size_t)ne * 2 * sizeof(int32_t), st) != hipSuccess)
                EMP_FAIL(EMP_ELAUNCH, "label_graph_index: memset failed");
        }
        return EMP_OK;
    }
    EMP_REQUIRE(vkeys && vdeg && work && vertices && objects && (ne == 0 || (ekeys && ecodes && edges)),
                "label_graph_index: null pointer");
    LtIndexWork L = lt_index_carve(work, nv);
    EMP_REQUIRE(work_bytes >= L.total, "label_graph_index: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    const int grid = emp_grid(nv, 256, 4096);
    int rc = emp_compact(
        L.head, nv, L.pos, L.scantmp, n_objects, stream, "label_graph_index: count copy",
        [&]() -> int {
            EMP_LAUNCH(lt_flags_kernel, grid, 256, st, vkeys, vdeg, nv, L.head, L.iso, L.end, L.junc);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(lt_objects_kernel, grid, 256, st, vkeys, nv, L.head, L.pos, ekeys, ne, H, W, vertices, objects,
                       max_objects);
            return EMP_OK;
        });
    if (rc != EMP_OK) return rc;
    if ((rc = emp_exclusive_scan_i32(L.iso, nv, L.p_iso, L.scantmp, stream)) != EMP_OK) return rc;
    if ((rc = emp_exclusive_scan_i32(L.end, nv, L.p_end, L.scantmp, stream)) != EMP_OK) return rc;
    if ((rc = emp_exclusive_scan_i32(L.junc, nv, L.p_junc, L.scantmp, stream)) != EMP_OK) return rc;
    EMP_LAUNCH(lt_object_counts_kernel, emp_grid(max_objects > 0 ? max_objects : 1, 256, 1024), 256, st, n_objects,
               max_objects, L.p_iso, L.p_end, L.p_junc, objects);
    if (ne > 0)
        EMP_LAUNCH(lt_edges_kernel, emp_grid(ne, 256, 4096), 256, st, ekeys, ecodes, ne, vkeys, objects, n_objects,
                   max_objects, H, W, edges);
    return EMP_OK;
}
