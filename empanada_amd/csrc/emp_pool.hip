// Mode pooling of label volumes: one level of a multiscale pyramid.  Output voxel (z, y, x) is the most frequent value
// of the input cell [fz z, fz z + fz) x [fy y, ...) x [fx x, ...) clipped to the volume, every factor 1 or 2; among
// values that occur equally often the largest (unsigned) wins.  Labels cannot be averaged, and neither torch nor the
// reference has this reduction (its viewers down-sample on the CPU after the volume has been written).
//
// A streaming pass in the form of emp_fuse_apply and row_runs_kernel: a lane owns 16 bytes of one output row (4
// uint32 or 16 uint8 voxels), reads their fx x 16 bytes from each of the fy * fz contributing input rows with 16-byte
// loads -- all of them issued before the first comparison -- and writes one 16-byte store.  Per output voxel it
// reads fz fy fx elements and writes one: that is the whole traffic, there is no workspace and no LDS.  The input is
// read exactly once, so the wide loads carry the non-temporal hint; the hint also keeps them what they are: without
// it the compiler folds the uint32 wide path into the element path (same values from the same addresses), and the
// pass runs on 4-byte loads at 53 % of a device copy instead of 93 % (profiles/label_pyramid.md).
//
// Clipped cells (odd sizes) need no validity mask.  A position past the volume is not read: its index is clamped to
// the last valid one along that axis, which for factors of 2 is the position's own partner, so every valid voxel of
// the cell is counted 2^(clipped axes) times.  Multiplying all counts by one number changes neither their order nor
// their ties, hence not the winner.
#include "emp_common.h"

// mode of N values, one cell: count[a] = number of OTHER values equal to v[a] (N (N - 1) / 2 comparisons, 28 for a full
// cell), result = value of the largest (count, value)
template <int N> __device__ __forceinline__ uint32_t pool_mode_scalar(const uint32_t (&v)[N])
{
    uint32_t c[N];
#pragma unroll
    for (int a = 0; a < N; ++a) c[a] = 0u;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a + 1; b < N; ++b) {
            const uint32_t e = v[a] == v[b] ? 1u : 0u;
            c[a] += e;
            c[b] += e;
        }
    uint64_t best = 0ull;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const uint64_t key = ((uint64_t)c[a] << 32) | (uint64_t)v[a];
        best = key > best ? key : best;
    }
    return (uint32_t)best;
}

// the same for four uint8 cells at once: byte k of w[a] is value a of cell k.  Equal bytes are found without carries
// between bytes (the classic zero-byte test on a ^ b), the counts (<= 7) are summed per byte, and (count, value) is
// compared as 16-bit keys count << 8 | value, two cells per register.
typedef unsigned short pool_us2 __attribute__((ext_vector_type(2)));
typedef uint32_t pool_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t pool_max_u16x2(uint32_t a, uint32_t b)
{
    const pool_us2 m = __builtin_elementwise_max(__builtin_bit_cast(pool_us2, a), __builtin_bit_cast(pool_us2, b));
    return __builtin_bit_cast(uint32_t, m);
}

template <int N> __device__ __forceinline__ uint32_t pool_mode_bytes(const uint32_t (&w)[N])
{
    uint32_t c[N];
#pragma unroll
    for (int a = 0; a < N; ++a) c[a] = 0u;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a + 1; b < N; ++b) {
            const uint32_t x = w[a] ^ w[b];
            // bit 7 of a byte of y is set iff that byte of x is not zero; the sum cannot carry out of a byte
            const uint32_t y = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
            const uint32_t e = (~y >> 7) & 0x01010101u;
            c[a] += e;
            c[b] += e;
        }
    uint32_t lo = 0u, hi = 0u;                       // cells 0 and 2, cells 1 and 3
#pragma unroll
    for (int a = 0; a < N; ++a) {
        lo = pool_max_u16x2(lo, ((c[a] & 0x00ff00ffu) << 8) | (w[a] & 0x00ff00ffu));
        hi = pool_max_u16x2(hi, (c[a] & 0xff00ff00u) | ((w[a] >> 8) & 0x00ff00ffu));
    }
    return (lo & 0x00ff00ffu) | ((hi & 0x00ff00ffu) << 8);
}

// Threads of a block: 2^lpr_log2 lanes side by side along x, 256 >> lpr_log2 output rows; blockIdx.x strides over the
// groups of rows, blockIdx.y over the lanes' positions along x, so the one division per row (z = r / Ho) is not paid
// per voxel.  wide_in / wide_out: every input / output row starts on a 16-byte address.  A lane whose 16 bytes (or
// their inputs) reach past the row's end, and every lane of an array whose rows are not aligned, takes the element
// loads and stores instead, into the same registers.
template <typename T, int FZ, int FY, int FX>
__global__ __launch_bounds__(256) void pool_mode_kernel(const T *__restrict__ src, int64_t D, int64_t H, int64_t W,
                                                        int64_t Do, int64_t Ho, int64_t Wo, T *__restrict__ dst,
                                                        int lpr_log2, int64_t G, int wide_in, int wide_out)
{
    constexpr int VO = 16 / (int)sizeof(T);          // output voxels of a lane
    constexpr int NR = FZ * FY;                      // input rows of an output row
    constexpr int NI = FX * VO;                      // input voxels of a lane per input row
    constexpr int ND = FX * 4;                       // ... in dwords
    constexpr int N = NR * FX;                       // values of a full cell
    const int64_t lpr = (int64_t)1 << lpr_log2;
    const int64_t rpb = 256 >> lpr_log2;
    const int64_t sub = threadIdx.x >> lpr_log2, gl = threadIdx.x & (lpr - 1);
    const int64_t R = Do * Ho, n_groups = (R + rpb - 1) / rpb;
    const bool small = R <= 0x7fffffffLL;            // uniform: 32-bit division where it is exact
    for (int64_t rg = blockIdx.x; rg < n_groups; rg += gridDim.x) {
        const int64_t r = rg * rpb + sub;
        if (r >= R) continue;
        const int64_t z = small ? (int64_t)((uint32_t)r / (uint32_t)Ho) : r / Ho;
        const int64_t y = r - z * Ho;
        const T *rows[NR];
#pragma unroll
        for (int dz = 0; dz < FZ; ++dz)
#pragma unroll
            for (int dy = 0; dy < FY; ++dy) {
                const int64_t zz = FZ * z + dz < D ? FZ * z + dz : D - 1;
                const int64_t yy = FY * y + dy < H ? FY * y + dy : H - 1;
                rows[dz * FY + dy] = src + (zz * H + yy) * W;
            }
        T *orow = dst + r * Wo;
        for (int64_t g = (int64_t)blockIdx.y * lpr + gl; g < G; g += (int64_t)gridDim.y * lpr) {
            const int64_t x0 = g * VO, xi = x0 * FX;
            uint32_t d[NR][ND];
            if (wide_in && xi + NI <= W) {
#pragma unroll
                for (int q = 0; q < NR; ++q)
#pragma unroll
                    for (int k = 0; k < FX; ++k) {
                        const pool_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const pool_u32x4 *>(rows[q] + xi + k * VO));
                        d[q][4 * k] = t.x; d[q][4 * k + 1] = t.y; d[q][4 * k + 2] = t.z; d[q][4 * k + 3] = t.w;
                    }
            } else {
#pragma unroll
                for (int q = 0; q < NR; ++q)
#pragma unroll
                    for (int m = 0; m < ND; ++m) {
                        if constexpr (sizeof(T) == 4) {
                            const int64_t x = xi + m < W ? xi + m : W - 1;
                            d[q][m] = (uint32_t)rows[q][x];
                        } else {
                            uint32_t word = 0u;
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const int64_t x = xi + 4 * m + b < W ? xi + 4 * m + b : W - 1;
                                word |= (uint32_t)rows[q][x] << (8 * b);
                            }
                            d[q][m] = word;
                        }
                    }
            }
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t v[N];
#pragma unroll
                for (int q = 0; q < NR; ++q) {
                    if constexpr (sizeof(T) == 4) {                     // output voxel j of the lane
#pragma unroll
                        for (int dx = 0; dx < FX; ++dx) v[q * FX + dx] = d[q][FX * j + dx];
                    } else if constexpr (FX == 1) {                     // output voxels 4j .. 4j + 3, one per byte
                        v[q] = d[q][j];
                    } else {                                            // even and odd bytes of 8 input voxels
                        v[q * 2] = __builtin_amdgcn_perm(d[q][2 * j + 1], d[q][2 * j], 0x06040200u);
                        v[q * 2 + 1] = __builtin_amdgcn_perm(d[q][2 * j + 1], d[q][2 * j], 0x07050301u);
                    }
                }
                if constexpr (sizeof(T) == 4) o[j] = pool_mode_scalar<N>(v);
                else o[j] = pool_mode_bytes<N>(v);
            }
            if (wide_out && x0 + VO <= Wo) {
                *reinterpret_cast<uint4 *>(orow + x0) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < VO; ++j) {
                    if (x0 + j < Wo) {
                        if constexpr (sizeof(T) == 4) orow[x0 + j] = (T)o[j];
                        else orow[x0 + j] = (T)((o[j >> 2] >> (8 * (j & 3))) & 0xffu);
                    }
                }
            }
        }
    }
}

template <typename T, int FZ, int FY, int FX>
static int pool_launch(const void *src, int64_t D, int64_t H, int64_t W, void *dst, hipStream_t st)
{
    constexpr int64_t VO = 16 / (int64_t)sizeof(T);
    const int64_t Do = emp_cdiv(D, FZ), Ho = emp_cdiv(H, FY), Wo = emp_cdiv(W, FX);
    const int64_t G = emp_cdiv(Wo, VO);              // lanes along an output row
    int lpr_log2 = 0;
    while (lpr_log2 < 8 && ((int64_t)1 << lpr_log2) < G) ++lpr_log2;
    const int64_t lpr = (int64_t)1 << lpr_log2, rpb = 256 >> lpr_log2;
    int64_t gy = emp_cdiv(G, lpr);
    if (gy > 1024) gy = 1024;                        // the rest of a very long row: the kernel's loop over g
    int64_t gx = emp_cdiv(Do * Ho, rpb);
    const int64_t cap = 16384 / gy > 1 ? 16384 / gy : 1;
    if (gx > cap) gx = cap;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
    const int wide_in = a % 16 == 0 && (W * (int64_t)sizeof(T)) % 16 == 0;
    const int wide_out = b % 16 == 0 && (Wo * (int64_t)sizeof(T)) % 16 == 0;
    hipLaunchKernelGGL((pool_mode_kernel<T, FZ, FY, FX>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st,
                       reinterpret_cast<const T *>(src), D, H, W, Do, Ho, Wo, reinterpret_cast<T *>(dst), lpr_log2, G,
                       wide_in, wide_out);
    EMP_CHECK_LAUNCH("pool_mode_kernel");
    return EMP_OK;
}

template <typename T> static int pool_dispatch(const void *src, int64_t D, int64_t H, int64_t W, int fz, int fy, int fx,
                                               void *dst, hipStream_t st)
{
    switch ((fz - 1) * 4 + (fy - 1) * 2 + (fx - 1)) {
    case 1: return pool_launch<T, 1, 1, 2>(src, D, H, W, dst, st);
    case 2: return pool_launch<T, 1, 2, 1>(src, D, H, W, dst, st);
    case 3: return pool_launch<T, 1, 2, 2>(src, D, H, W, dst, st);
    case 4: return pool_launch<T, 2, 1, 1>(src, D, H, W, dst, st);
    case 5: return pool_launch<T, 2, 1, 2>(src, D, H, W, dst, st);
    case 6: return pool_launch<T, 2, 2, 1>(src, D, H, W, dst, st);
    default: return pool_launch<T, 2, 2, 2>(src, D, H, W, dst, st);
    }
}

extern "C" int emp_label_pool_mode(const void *src, int item, int64_t D, int64_t H, int64_t W, int fz, int fy, int fx,
                                   void *dst, void *stream)
{
    EMP_REQUIRE(item == 1 || item == 4, "label_pool_mode: item must be 1 (uint8) or 4 (uint32), got %d", item);
    EMP_REQUIRE((fz == 1 || fz == 2) && (fy == 1 || fy == 2) && (fx == 1 || fx == 2),
                "label_pool_mode: every factor must be 1 or 2, got (%d, %d, %d)", fz, fy, fx);
    EMP_REQUIRE(fz * fy * fx > 1, "label_pool_mode: factors (1, 1, 1) pool nothing");
    EMP_REQUIRE(D >= 0 && H >= 0 && W >= 0, "label_pool_mode: negative size (%lld, %lld, %lld)", (long long)D,
                (long long)H, (long long)W);
    if (D == 0 || H == 0 || W == 0) return EMP_OK;
    EMP_REQUIRE(H <= INT64_MAX / 8 / D && W <= INT64_MAX / 8 / (D * H),
                "label_pool_mode: (%lld, %lld, %lld) voxels do not fit 64-bit byte offsets", (long long)D, (long long)H,
                (long long)W);
    EMP_REQUIRE(src && dst, "label_pool_mode: null pointer");
    EMP_REQUIRE(reinterpret_cast<uintptr_t>(src) % (uintptr_t)item == 0 &&
                    reinterpret_cast<uintptr_t>(dst) % (uintptr_t)item == 0, "label_pool_mode: misaligned labels");
    hipStream_t st = emp_stream(stream);
    if (item == 4) return pool_dispatch<uint32_t>(src, D, H, W, fz, fy, fx, dst, st);
    return pool_dispatch<uint8_t>(src, D, H, W, fz, fy, fx, dst, st);
}
