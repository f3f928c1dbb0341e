// Geodesic growth of seeds inside the objects of a label volume (include/emp_hip.h, E6): every labelled voxel is given
// to the seed that reaches it first along 6-connected paths that stay inside the voxel's own label, the largest seed id
// among equally near ones.  The flood of a watershed on a binary mask, which users of the reference run on a CPU; the
// definition is the header's.
//
// State: one aligned 64-bit key per voxel, dist << 32 | ~owner, all-ones = not reached.  Keys only fall, and a key that
// is stored is always one that some schedule of the min-relaxation could have produced, so a block may read a neighbour
// tile's keys while that tile's block rewrites them: it sees the old key or the new one, never half of one, and either
// is an upper bound of the fixed point.  A sweep after which no block has stored anything has read only settled keys.
//
// Tile: 8 x 8 x 64 voxels (x fastest: a row of the tile is 512 B of keys) and 256 threads, 16 voxels each.  The keys
// of the tile and of its one-voxel ring take 10 x 10 x 66 x 8 = 52 800 B of LDS; the labels never stay there: they are
// staged in the same bytes, reduced to one byte per voxel that says which of the six neighbours carry the voxel's
// label, and the keys are loaded over them.  56.9 KB per block leaves two blocks per CU.  The relaxation is Jacobi --
// every thread reads, a barrier, every thread writes, a barrier that also votes -- so no 64-bit LDS word is read
// while it is written.
//
// Work per sweep follows the tiles that can still change: emp_label_grow_init lists the tiles that hold a labelled
// voxel and marks as due those that hold a seed or face one; a block of a tile that is not due leaves at once; a block
// that lowers a key on a face of its tile marks the tile behind that face as due for the next sweep.  The marks are
// bytes in two arrays that take turns, written with plain stores of 1.  Nothing is atomic but the list's length in the
// initialisation and the counter of blocks that stored something.  No block waits on another.
#include "emp_common.h"

#define LG_TZ EMP_TILE_Z
#define LG_TY EMP_TILE_Y
#define LG_TX EMP_TILE_X
#define LG_PZ (LG_TZ + 2)
#define LG_PY (LG_TY + 2)
#define LG_PX (LG_TX + 2)
#define LG_CELLS (LG_PZ * LG_PY * LG_PX)
#define LG_VOX (LG_TZ * LG_TY * LG_TX)
#define LG_THREADS 256
#define LG_PER (LG_VOX / LG_THREADS)
#define LG_SLOTS 8
#define LG_NONE 0xffffffffffffffffULL
#define LG_STEP (1ULL << 32)

typedef unsigned long long lg_key;

// counters[0]: length of the list; counters[1 + slot]: blocks that stored something in the sweeps given that slot
struct LgWork {
    lg_key *counters;
    int32_t *list;
    uint8_t *due[2];
    int64_t total;
};
static LgWork lg_carve(void *work, int64_t n_tiles)
{
    if (n_tiles < 1) n_tiles = 1;
    EmpCarver c(work);
    LgWork L;
    L.counters = c.take<lg_key>(1 + LG_SLOTS);
    L.list = c.take<int32_t>(n_tiles);
    L.due[0] = c.take<uint8_t>(n_tiles);
    L.due[1] = c.take<uint8_t>(n_tiles);
    L.total = c.bytes();
    return L;
}

extern "C" int64_t emp_label_grow_work_bytes(int64_t D, int64_t H, int64_t W)
{
    if (!emp_tiles_shape_ok(D, H, W)) return -1;
    return lg_carve(nullptr, emp_tiles(D, H, W).n).total;
}

__global__ void lg_clear_kernel(int64_t n_tiles, lg_key *__restrict__ counters, uint8_t *__restrict__ due0,
                                uint8_t *__restrict__ due1)
{
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 < 1 + LG_SLOTS) counters[i0] = 0;
    for (int64_t i = i0; i < n_tiles; i += (int64_t)gridDim.x * blockDim.x) due0[i] = due1[i] = 0;
}

// bits of a tile's report: 0 the tile itself, 1 .. 6 the tiles behind its faces -z +z -y +y -x +x
__device__ __forceinline__ int lg_face_bits(int lz, int ly, int lx)
{
    return 1 | (lz == 0 ? 2 : 0) | (lz == LG_TZ - 1 ? 4 : 0) | (ly == 0 ? 8 : 0) | (ly == LG_TY - 1 ? 16 : 0) |
           (lx == 0 ? 32 : 0) | (lx == LG_TX - 1 ? 64 : 0);
}

__device__ __forceinline__ void lg_mark(int bits, int64_t tz, int64_t ty, int64_t tx, EmpTiles T, int64_t tile,
                                        uint8_t *due)
{
    if (bits & 1) due[tile] = 1;
    if ((bits & 2) && tz > 0) due[tile - T.ny * T.nx] = 1;
    if ((bits & 4) && tz + 1 < T.nz) due[tile + T.ny * T.nx] = 1;
    if ((bits & 8) && ty > 0) due[tile - T.nx] = 1;
    if ((bits & 16) && ty + 1 < T.ny) due[tile + T.nx] = 1;
    if ((bits & 32) && tx > 0) due[tile - 1] = 1;
    if ((bits & 64) && tx + 1 < T.nx) due[tile + 1] = 1;
}

template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_init_kernel(const T *__restrict__ lab, const uint32_t *__restrict__ seeds,
                                                             int64_t D, int64_t H, int64_t W, EmpTiles tiles,
                                                             lg_key *__restrict__ state, lg_key *counters,
                                                             int32_t *__restrict__ list, uint8_t *due)
{
    __shared__ int s_bits, s_lab;
    for (int64_t tile = blockIdx.x; tile < tiles.n; tile += gridDim.x) {
        if (threadIdx.x == 0) s_bits = s_lab = 0;
        __syncthreads();
        const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
        int bits = 0, any = 0;
        for (int i = threadIdx.x; i < LG_VOX; i += LG_THREADS) {
            const int lx = i & (LG_TX - 1), ly = (i / LG_TX) & (LG_TY - 1), lz = i / (LG_TX * LG_TY);
            const int64_t z = tz * LG_TZ + lz, y = ty * LG_TY + ly, x = tx * LG_TX + lx;
            if (z >= D || y >= H || x >= W) continue;
            const int64_t at = (z * H + y) * W + x;
            const uint32_t l = (uint32_t)lab[at], s = seeds[at];
            lg_key key = LG_NONE;
            if (l != 0) {
                any = 1;
                if (s != 0) {
                    key = (lg_key)(~s);
                    bits |= lg_face_bits(lz, ly, lx);
                }
            }
            state[at] = key;
        }
        if (bits) atomicOr(&s_bits, bits);
        if (any) atomicOr(&s_lab, 1);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (s_lab) list[atomicAdd(counters, 1ULL)] = (int32_t)tile;
            lg_mark(s_bits, tz, ty, tx, tiles, tile, due);
        }
        __syncthreads();
    }
}

#define LG_REQUIRE_SHAPE(what)                                                                                         \
    do {                                                                                                               \
        EMP_REQUIRE_VOLUME(what);                                                                                      \
        EMP_REQUIRE(emp_tiles_shape_ok(D, H, W),                                                                       \
                    what ": %lld x %lld x %lld voxels are more than 2^31 - 1; cut the slab into z-blocks",             \
                    (long long)D, (long long)H, (long long)W);                                                         \
    } while (0)

extern "C" int emp_label_grow_init(const void *lab, int item, const uint32_t *seeds, int64_t D, int64_t H, int64_t W,
                                   uint64_t *state, void *work, int64_t work_bytes, void *stream)
{
    LG_REQUIRE_SHAPE("label_grow_init");
    EMP_REQUIRE(work, "label_grow_init: null pointer");
    const EmpTiles T = emp_tiles(D, H, W);
    LgWork L = lg_carve(work, T.n);
    EMP_REQUIRE(work_bytes >= L.total, "label_grow_init: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    EMP_LAUNCH(lg_clear_kernel, emp_grid(T.n > 16 ? T.n : 16, 256, 1024), 256, st, T.n, L.counters, L.due[0], L.due[1]);
    if (D == 0) return EMP_OK;
    EMP_REQUIRE(lab && seeds && state, "label_grow_init: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 && (reinterpret_cast<uintptr_t>(seeds) % 4) == 0 &&
                    (reinterpret_cast<uintptr_t>(state) % 8) == 0,
                "label_grow_init: misaligned pointer");
    lg_key *keys = reinterpret_cast<lg_key *>(state);
    const int grid = emp_grid(T.n, 1, 16384);
    if (item == 4)
        EMP_LAUNCH((lg_init_kernel<uint32_t>), grid, LG_THREADS, st, reinterpret_cast<const uint32_t *>(lab), seeds, D, H, W,
                   T, keys, L.counters, L.list, L.due[0]);
    else
        EMP_LAUNCH((lg_init_kernel<uint8_t>), grid, LG_THREADS, st, reinterpret_cast<const uint8_t *>(lab), seeds, D, H, W,
                   T, keys, L.counters, L.list, L.due[0]);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ sweep
template <typename T>
struct LgHalo {
    const T *lab_below, *lab_above;          // one (H, W) slice each, null = the volume's face
    const lg_key *key_below, *key_above;
};

__device__ __forceinline__ lg_key lg_peek(const lg_key *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ lg_key lg_next(lg_key c)
{
    const lg_key n = c + LG_STEP;
    return n < c ? LG_NONE : n;               // all-ones stays all-ones
}

template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_sweep_kernel(const T *__restrict__ lab, int64_t D, int64_t H, int64_t W,
                                                              EmpTiles tiles, LgHalo<T> halo, lg_key *state,
                                                              const int32_t *__restrict__ list, uint8_t *due_now,
                                                              uint8_t *due_next, int force, lg_key *counter)
{
    __shared__ lg_key s_key[LG_CELLS];
    __shared__ uint8_t s_same[LG_VOX];
    __shared__ int s_bits;
    const int64_t tile = list[blockIdx.x];
    const int64_t tx = tile % tiles.nx, ty = (tile / tiles.nx) % tiles.ny, tz = tile / (tiles.nx * tiles.ny);
    const bool run = due_now[tile] || ((force & 1) && tz == 0) || ((force & 2) && tz + 1 == tiles.nz);
    if (threadIdx.x == 0) s_bits = 0;
    __syncthreads();                              // every thread has read the mark before it is taken back
    if (threadIdx.x == 0) due_now[tile] = 0;
    if (!run) return;
    const int64_t z0 = tz * LG_TZ - 1, y0 = ty * LG_TY - 1, x0 = tx * LG_TX - 1;

    // 1. the labels of the tile and its ring, staged in the bytes that the keys take afterwards; 0 outside the volume
    uint32_t *s_lab = reinterpret_cast<uint32_t *>(s_key);
    for (int c = threadIdx.x; c < LG_CELLS; c += LG_THREADS) {
        const int px = c % LG_PX, py = (c / LG_PX) % LG_PY, pz = c / (LG_PX * LG_PY);
        const int64_t z = z0 + pz, y = y0 + py, x = x0 + px;
        uint32_t l = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            if (z >= 0 && z < D) l = (uint32_t)lab[(z * H + y) * W + x];
            else if (z == -1 && halo.lab_below) l = (uint32_t)halo.lab_below[y * W + x];
            else if (z == D && halo.lab_above) l = (uint32_t)halo.lab_above[y * W + x];
        }
        s_lab[c] = l;
    }
    __syncthreads();
    // 2. which neighbours carry the voxel's own label: bits 0 .. 5 = -z +z -y +y -x +x
    int mine = 0;
    for (int k = 0; k < LG_PER; ++k) {
        const int i = threadIdx.x + k * LG_THREADS;
        const int lx = i & (LG_TX - 1), ly = (i / LG_TX) & (LG_TY - 1), lz = i / (LG_TX * LG_TY);
        const int c = ((lz + 1) * LG_PY + ly + 1) * LG_PX + lx + 1;
        const uint32_t l = s_lab[c];
        int m = 0;
        // a tile that overhangs the slab's last slice holds the `above` slice at lz = D - z: that cell is ring, not tile
        if (l != 0 && z0 + 1 + lz < D) {
            m = (s_lab[c - LG_PY * LG_PX] == l ? 1 : 0) | (s_lab[c + LG_PY * LG_PX] == l ? 2 : 0) |
                (s_lab[c - LG_PX] == l ? 4 : 0) | (s_lab[c + LG_PX] == l ? 8 : 0) | (s_lab[c - 1] == l ? 16 : 0) |
                (s_lab[c + 1] == l ? 32 : 0);
        }
        s_same[i] = (uint8_t)m;
        mine |= m;
    }
    __syncthreads();
    // 3. the keys: the tile's own are this block's alone to write; the ring's are read as they are at this moment
    for (int c = threadIdx.x; c < LG_CELLS; c += LG_THREADS) {
        const int px = c % LG_PX, py = (c / LG_PX) % LG_PY, pz = c / (LG_PX * LG_PY);
        const int64_t z = z0 + pz, y = y0 + py, x = x0 + px;
        lg_key key = LG_NONE;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            if (z >= 0 && z < D) key = lg_peek(state + (z * H + y) * W + x);
            else if (z == -1 && halo.key_below) key = lg_peek(halo.key_below + y * W + x);
            else if (z == D && halo.key_above) key = lg_peek(halo.key_above + y * W + x);
        }
        s_key[c] = key;
    }
    __syncthreads();
    // 4. relax until nothing in the tile changes
    unsigned lowered = 0;
    int again = __syncthreads_or(mine);
    while (again) {
        lg_key best[LG_PER];
        unsigned now = 0;
#pragma unroll
        for (int k = 0; k < LG_PER; ++k) {
            const int i = threadIdx.x + k * LG_THREADS;
            const int m = s_same[i];
            best[k] = LG_NONE;
            if (m == 0) continue;
            const int lx = i & (LG_TX - 1), ly = (i / LG_TX) & (LG_TY - 1), lz = i / (LG_TX * LG_TY);
            const int c = ((lz + 1) * LG_PY + ly + 1) * LG_PX + lx + 1;
            const lg_key old = s_key[c];
            lg_key b = old;
            if (m & 1) b = min(b, lg_next(s_key[c - LG_PY * LG_PX]));
            if (m & 2) b = min(b, lg_next(s_key[c + LG_PY * LG_PX]));
            if (m & 4) b = min(b, lg_next(s_key[c - LG_PX]));
            if (m & 8) b = min(b, lg_next(s_key[c + LG_PX]));
            if (m & 16) b = min(b, lg_next(s_key[c - 1]));
            if (m & 32) b = min(b, lg_next(s_key[c + 1]));
            best[k] = b;
            if (b < old) now |= 1u << k;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LG_PER; ++k) {
            if (now & (1u << k)) {
                const int i = threadIdx.x + k * LG_THREADS;
                const int lx = i & (LG_TX - 1), ly = (i / LG_TX) & (LG_TY - 1), lz = i / (LG_TX * LG_TY);
                s_key[((lz + 1) * LG_PY + ly + 1) * LG_PX + lx + 1] = best[k];
            }
        }
        lowered |= now;
        again = __syncthreads_or((int)now);
    }
    // 5. the lowered keys go back, and the tiles behind the faces they lie on are due next
    int bits = 0;
    for (int k = 0; k < LG_PER; ++k) {
        if (!(lowered & (1u << k))) continue;
        const int i = threadIdx.x + k * LG_THREADS;
        const int lx = i & (LG_TX - 1), ly = (i / LG_TX) & (LG_TY - 1), lz = i / (LG_TX * LG_TY);
        const int64_t z = z0 + 1 + lz, y = y0 + 1 + ly, x = x0 + 1 + lx;      // inside the volume: its label is not 0
        __hip_atomic_store(state + (z * H + y) * W + x, s_key[((lz + 1) * LG_PY + ly + 1) * LG_PX + lx + 1],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bits |= lg_face_bits(lz, ly, lx);
    }
    if (bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0 && s_bits) {
        atomicAdd(counter, 1ULL);
        lg_mark(s_bits & ~1, tz, ty, tx, tiles, tile, due_next);
    }
}

extern "C" int emp_label_grow_sweep(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint64_t *state,
                                    const void *below_lab, const uint64_t *below_state, const void *above_lab,
                                    const uint64_t *above_state, void *work, int64_t work_bytes, int64_t n_listed,
                                    int turn, int force, int slot, void *stream)
{
    LG_REQUIRE_SHAPE("label_grow_sweep");
    EMP_REQUIRE((below_lab == nullptr) == (below_state == nullptr) && (above_lab == nullptr) == (above_state == nullptr),
                "label_grow_sweep: a halo is one slice of labels AND one of state, or neither");
    EMP_REQUIRE((turn == 0 || turn == 1) && force >= 0 && force <= 3 && slot >= 0 && slot < LG_SLOTS,
                "label_grow_sweep: turn = %d, force = %d, slot = %d outside 0 .. 1, 0 .. 3, 0 .. %d", turn, force, slot,
                LG_SLOTS - 1);
    const EmpTiles T = emp_tiles(D, H, W);
    EMP_REQUIRE(n_listed >= 0 && n_listed <= T.n, "label_grow_sweep: %lld listed tiles, the slab has %lld",
                (long long)n_listed, (long long)T.n);
    if (D == 0 || n_listed == 0) return EMP_OK;
    EMP_REQUIRE(lab && state && work, "label_grow_sweep: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(state) % 8) == 0 && (reinterpret_cast<uintptr_t>(below_state) % 8) == 0 &&
                    (reinterpret_cast<uintptr_t>(above_state) % 8) == 0 &&
                    (reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0 &&
                    (reinterpret_cast<uintptr_t>(below_lab) % (uintptr_t)item) == 0 &&
                    (reinterpret_cast<uintptr_t>(above_lab) % (uintptr_t)item) == 0,
                "label_grow_sweep: misaligned pointer");
    LgWork L = lg_carve(work, T.n);
    EMP_REQUIRE(work_bytes >= L.total, "label_grow_sweep: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    lg_key *keys = reinterpret_cast<lg_key *>(state);
    if (item == 4) {
        LgHalo<uint32_t> halo = {reinterpret_cast<const uint32_t *>(below_lab), reinterpret_cast<const uint32_t *>(above_lab),
                                 reinterpret_cast<const lg_key *>(below_state),
                                 reinterpret_cast<const lg_key *>(above_state)};
        EMP_LAUNCH((lg_sweep_kernel<uint32_t>), (int)n_listed, LG_THREADS, st, reinterpret_cast<const uint32_t *>(lab), D, H,
                   W, T, halo, keys, L.list, L.due[turn], L.due[1 - turn], force, L.counters + 1 + slot);
    } else {
        LgHalo<uint8_t> halo = {reinterpret_cast<const uint8_t *>(below_lab), reinterpret_cast<const uint8_t *>(above_lab),
                                reinterpret_cast<const lg_key *>(below_state),
                                reinterpret_cast<const lg_key *>(above_state)};
        EMP_LAUNCH((lg_sweep_kernel<uint8_t>), (int)n_listed, LG_THREADS, st, reinterpret_cast<const uint8_t *>(lab), D, H, W,
                   T, halo, keys, L.list, L.due[turn], L.due[1 - turn], force, L.counters + 1 + slot);
    }
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ paint
// mode 0: dst = owner ? lut[owner] : lab, written only where it differs when dst is lab itself; mode 1: dst = owner
template <typename T, typename O>
__global__ void lg_paint_kernel(int64_t n, const lg_key *__restrict__ state, const T *lab, const uint32_t *__restrict__ lut,
                                int64_t n_lut, int mode, int in_place, O *dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t owner = ~(uint32_t)state[i];
        if (mode == 1) {
            dst[i] = (O)owner;
            continue;
        }
        const uint32_t l = (uint32_t)lab[i];
        const uint32_t v = (owner != 0 && (int64_t)owner < n_lut) ? lut[owner] : l;
        if (!in_place || v != l) dst[i] = (O)v;
    }
}

extern "C" int emp_label_grow_paint(const uint64_t *state, const void *lab, int item, int64_t n, const uint32_t *lut,
                                    int64_t n_lut, int mode, void *dst, int dst_item, void *stream)
{
    EMP_REQUIRE(item == 1 || item == 4, "label_grow_paint: labels must be uint8 (1) or uint32 (4), got %d bytes", item);
    EMP_REQUIRE(dst_item == 1 || dst_item == 4, "label_grow_paint: dst must be uint8 (1) or uint32 (4), got %d bytes",
                dst_item);
    EMP_REQUIRE(mode == 0 || (mode == 1 && dst_item == 4), "label_grow_paint: mode %d with a %d-byte dst", mode, dst_item);
    EMP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "label_grow_paint: %lld voxels outside 0 .. 2^31 - 1", (long long)n);
    EMP_REQUIRE(n_lut >= 0 && n_lut <= (1LL << 32), "label_grow_paint: %lld lut entries", (long long)n_lut);
    if (n == 0) return EMP_OK;
    EMP_REQUIRE(state && dst && (mode == 1 || lab) && (mode == 1 || n_lut == 0 || lut), "label_grow_paint: null pointer");
    EMP_REQUIRE((reinterpret_cast<uintptr_t>(state) % 8) == 0 && (reinterpret_cast<uintptr_t>(dst) % (uintptr_t)dst_item) == 0,
                "label_grow_paint: misaligned pointer");
    const char *l0 = reinterpret_cast<const char *>(lab), *l1 = l0 + n * item;
    const char *d0 = reinterpret_cast<const char *>(dst), *d1 = d0 + n * dst_item;
    const bool in_place = mode == 0 && d0 == l0 && dst_item == item;
    EMP_REQUIRE(mode == 1 || in_place || d1 <= l0 || d0 >= l1,
                "label_grow_paint: dst overlaps the labels without being the labels themselves");
    const char *s0 = reinterpret_cast<const char *>(state), *s1 = s0 + n * 8;
    EMP_REQUIRE(d1 <= s0 || d0 >= s1, "label_grow_paint: dst overlaps the state");
    hipStream_t st = emp_stream(stream);
    const lg_key *keys = reinterpret_cast<const lg_key *>(state);
    const int grid = emp_grid(n, 256, 16384);
    const int ip = in_place ? 1 : 0;
    if (item == 4 && dst_item == 4)
        EMP_LAUNCH((lg_paint_kernel<uint32_t, uint32_t>), grid, 256, st, n, keys, reinterpret_cast<const uint32_t *>(lab), lut,
                   n_lut, mode, ip, reinterpret_cast<uint32_t *>(dst));
    else if (item == 4)
        EMP_LAUNCH((lg_paint_kernel<uint32_t, uint8_t>), grid, 256, st, n, keys, reinterpret_cast<const uint32_t *>(lab), lut,
                   n_lut, mode, ip, reinterpret_cast<uint8_t *>(dst));
    else if (dst_item == 4)
        EMP_LAUNCH((lg_paint_kernel<uint8_t, uint32_t>), grid, 256, st, n, keys, reinterpret_cast<const uint8_t *>(lab), lut,
                   n_lut, mode, ip, reinterpret_cast<uint32_t *>(dst));
    else
        EMP_LAUNCH((lg_paint_kernel<uint8_t, uint8_t>), grid, 256, st, n, keys, reinterpret_cast<const uint8_t *>(lab), lut,
                   n_lut, mode, ip, reinterpret_cast<uint8_t *>(dst));
    return EMP_OK;
}
