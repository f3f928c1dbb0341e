// D4: implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) with the BatchNorm / residual /
// ReLU epilogue fused into the accumulator write-back.  gfx950 only.
//
//   GEMM view: M = N*OH*OW output pixels, N = Cout, K = KH*KW*Cin.  NHWC activations make every K-slab (16 or 32
//   input channels of one filter tap) of an A row contiguous; weights are stored (Cout, KH, KW, Cin) so a B row's
//   slab is contiguous as well.
//   Block = 256 threads = 2x2 waves, block tile 128 (pixels) x 128 (couts; 64 for narrow layers); each wave owns
//   64x64 = 2x2 MFMA tiles of 32x32 (4 accumulators x 16 VGPRs).  One barrier per K-slab.
//   Staging, two variants (template flag GLDS):
//     LDS-direct (default): global_load_lds_dwordx4, unpadded lane-linear LDS rows with a source-side XOR swizzle,
//       ring of 3 slabs (BK = 16, three blocks per CU) or 2 (BK = 32), counted vmcnt before a raw barrier;
//     global -> registers -> LDS (fused Winograd loader, EMP_CONV_NO_GLDS): LDS rows padded by 4 floats so
//       that the 16-byte fragment reads of 16 consecutive lanes cover all 64 banks exactly once; the loads of slab
//       s+2 are issued and slab s+1 is written to LDS between the MFMAs of slab s.
//   K order inside a slab of BK channels: the MFMA k-step j consumes channels j (lanes 0-31) and BK/2 + j (lanes
//   32-63), so a lane's operands are contiguous in LDS (ds_read_b128) -- see emp_hip.h for the resulting summation
//   order, which the oracle reproduces bit for bit.
//   blockIdx -> tile: consecutive hardware block ids go to different XCDs; tiles are renumbered so that each XCD
//   (its own L2) works on a contiguous range of tiles, cout-tiles fastest, and the A slabs shared by the cout
//   tiles of one pixel tile are fetched once per XCD.
#include "emp_common.h"
#include "emp_wino4.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CG_BM 128
#define CG_BK 32          // K granularity every entry point requires of Cin / K
#define CG_THREADS 256

struct ConvGeom {
    const float *x, *w, *scale, *shift, *res;
    float *out;
    int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, dil, relu;
    int64_t M, out_ps, res_ps;
    int tiles_m, tiles_n;
    int64_t x_bs, w_bs, out_bs;      // blockIdx.y batches (Winograd positions): element strides of x, w, out
    const int32_t *tiles;            // MODE 1: (M, 3) Winograd tile table
    const float *proj_w;             // PROJ: (proj_n, Cout) weights of a following 1x1 convolution to a few channels
    float *proj_out;                 // PROJ: planar (N, proj_n, hw) accumulator, zeroed by the caller
    int proj_n;
    int64_t hw;                      // PROJ: pixels per image
};

// 64 floats of zeros: the source of rows that fall outside the problem (padding taps, rows past M, couts past Cout)
// for the LDS-direct loader, which cannot mask data in flight
__device__ __attribute__((aligned(16))) float cg_zero_page[64];

// 16 bytes per lane from global memory straight into LDS (gfx950 global_load_lds_dwordx4): lane l's data lands at
// lds_byte_addr + 16 * l whatever its source address.  Not tracked by the compiler: pair with cg_wait_vm.
__device__ __forceinline__ void cg_glds16(const float *src, unsigned lds_byte_addr)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_byte_addr) : "memory", "m0");
}

template <int N>
__device__ __forceinline__ void cg_wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// NT = 32-wide cout tiles per wave: block tile 128 x (64 * NT) (NT = 1 for layers with Cout <= 64)
// MODE 0: A rows are output pixels of a convolution (implicit GEMM over filter taps).
// MODE 1: A rows are Winograd tiles and blockIdx.y is the position p = 4u + v; the loader fetches the four patch
//         pixels position p combines and applies the input transform on the way into LDS, so V never exists in
//         memory:  V_p = op_u(op_v(d[a0][b0], d[a0][b1]), op_v(d[a1][b0], d[a1][b1])), same roundings as
//         wino_input_kernel.
// RESPF: the residual values of the thread's epilogue rows are requested before the K loop (registers), so their
//        HBM latency hides behind the matrix work instead of sitting in the epilogue (short-K 1x1 convs).
// BK:    K-slab per barrier.  32: 64 MFMAs per wave between barriers, 72 KiB of LDS, 2 blocks per CU.
//        16: 32 MFMAs between barriers, 40 KiB of LDS and <= 168 VGPRs, 3 blocks per CU: the prologue / epilogue of
//        one block (global latency, LDS staging, stores) hides behind the matrix work of two others -- better for
//        short K loops.  Inside a slab the k-step j consumes channels j and BK/2 + j.
// PROJ:  the epilogue also feeds a following 1x1 convolution to a few channels (the heads' last layer): per row and
//        output channel q, lane partial ((v0 w0 + v1 w1) + v2 w2) + v3 w3 over its 4 couts, parked in LDS and summed
//        over the row's BN/4 lanes in ascending order, one atomicAdd per (row, q, cout tile) into a zeroed planar
//        accumulator.  With at most two cout tiles the result does not depend on the order of the atomics
//        (0 + a + b == 0 + b + a).  The activation itself need not be written (out == NULL).
// GATE:  epilogue out = residual * sigmoid(acc * scale + shift) (the per-pixel squeeze-excite of the RegNet blocks; a
//        template flag, not a run-time branch: a branch in the shared epilogue cost the residual-prefetch variant 3-5 %)
// GLDS:  the K-slabs go from global memory straight into LDS (no staging registers, no ds_write, no masking: invalid
//        rows read a zero page).  The LDS image of a slab is lane-linear, i.e. unpadded rows; bank conflicts of the
//        16-byte fragment reads are avoided by XOR-swizzling the 16-byte chunk index with the row ON THE SOURCE SIDE
//        (lane of physical chunk p fetches logical chunk p ^ f(row); a reader of logical chunk c looks at c ^ f(row)).
//        Ring of 3 slabs for BK = 16 (loads run two slabs ahead, `s_waitcnt vmcnt(loads of one slab)` before the
//        barrier), 2 for BK = 32.  Measured motivation: without the register -> LDS stage the same loop runs at 96 %
//        of the matrix peak instead of 83 %.
template <int NT, int MODE, bool RESPF = false, int BK = 32, bool PROJ = false, bool GLDS = false, bool GATE = false>
__global__ __launch_bounds__(CG_THREADS, (BK == 16 ? 3 : 2)) void conv_igemm_f32_kernel(ConvGeom g)
{
    constexpr int BN = 64 * NT;
    constexpr int CG_LD = GLDS ? BK : BK + 4;      // LDS row (floats): padded (register staging) or swizzled (GLDS)
    constexpr int NBUF = GLDS ? (BK == 16 ? 3 : 2) : 2;
    constexpr int TPR = BK / 4;                    // threads staging one row (one float4 each)
    constexpr int RPP = CG_THREADS / TPR;          // rows staged per pass
    constexpr int AR = CG_BM / RPP;                // A rows staged per thread
    constexpr int BROWS = BN / RPP;                // B rows staged per thread
    constexpr int NF4 = BK / 8;                    // float4 fragments per lane, tile and slab
    constexpr int CLD = BN + 4;                    // padded row of the epilogue staging tile (floats)
    constexpr int A_ELEMS = NBUF * CG_BM * CG_LD, B_ELEMS = NBUF * BN * CG_LD;
    constexpr int EPI_ROWS = (A_ELEMS + B_ELEMS >= CG_BM * CLD) ? CG_BM : 64;   // epilogue staged in 1 or 2 rounds
    constexpr int C_ELEMS = EPI_ROWS * CLD;
    constexpr int SMEM = (A_ELEMS + B_ELEMS) > C_ELEMS ? (A_ELEMS + B_ELEMS) : C_ELEMS;
    static_assert(MODE == 0 || BK == 32, "the fused Winograd loader is written for BK = 32");
    static_assert(!GLDS || MODE == 0, "LDS-direct staging: plain convolution / GEMM loader only");
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float *As = smem, *Bs = smem + A_ELEMS;
    g.x += (int64_t)blockIdx.y * g.x_bs;
    g.w += (int64_t)blockIdx.y * g.w_bs;
    g.out += (int64_t)blockIdx.y * g.out_bs;

    // XCD-aware tile numbering
    const int T = g.tiles_m * g.tiles_n;
    const int chunk = (T + 7) >> 3;
    const int tile = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (tile >= T) return;
    const int tm = tile / g.tiles_n, tn = tile % g.tiles_n;
    const int64_t m0 = (int64_t)tm * CG_BM;
    const int n0 = tn * BN;

    const int tid = threadIdx.x;
    const int lrow = tid / TPR, lcol = (tid % TPR) * 4;

    // the 4 A rows (output pixels / Winograd tiles) and BROWS B rows (couts) this thread stages, fixed over the K loop
    int a_n[AR], a_iy[AR], a_ix[AR];
    bool a_ok[AR], b_ok[BROWS];
    const float *b_ptr[BROWS];
    const int taps = g.KH * g.KW;
    int w_off[4][4];                   // MODE 1: element offsets of the 4 patch pixels of each row (0 when masked)
    unsigned w_mask[4];                // MODE 1: bit k set = pixel k inside the image
    float w_su = 1.f, w_sv = 1.f;      // MODE 1: sign of the second operand of the row / column combination
    if constexpr (MODE == 0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int64_t p = m0 + lrow + RPP * i;
            a_ok[i] = p < g.M;
            const int64_t pp = a_ok[i] ? p : 0;
            const int ox = (int)(pp % g.OW);
            const int oy = (int)((pp / g.OW) % g.OH);
            a_n[i] = (int)(pp / ((int64_t)g.OW * g.OH));
            a_iy[i] = oy * g.stride - g.pad;
            a_ix[i] = ox * g.stride - g.pad;
        }
    } else {
        // B^T rows: u = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
        const int u = blockIdx.y >> 2, v = blockIdx.y & 3;
        const int af = (u == 0) ? 0 : (u == 2) ? 2 : 1, as2 = (u == 0) ? 2 : (u == 1) ? 2 : (u == 2) ? 1 : 3;
        const int bf = (v == 0) ? 0 : (v == 2) ? 2 : 1, bs2 = (v == 0) ? 2 : (v == 1) ? 2 : (v == 2) ? 1 : 3;
        w_su = (u == 1) ? 1.f : -1.f;
        w_sv = (v == 1) ? 1.f : -1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t t = m0 + lrow + 32 * i;
            const bool ok = t < g.M;
            const int64_t tt = ok ? t : 0;
            const int n = g.tiles[3 * tt], by = g.tiles[3 * tt + 1], bx = g.tiles[3 * tt + 2];
            w_mask[i] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int yy = by + ((k >> 1) ? as2 : af) * g.dil, xx = bx + ((k & 1) ? bs2 : bf) * g.dil;
                const bool in = ok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
                w_off[i][k] = in ? (((n * g.H + yy) * g.W + xx) * g.Cin + lcol) : lcol;
                w_mask[i] |= in ? (1u << k) : 0u;
            }
            a_ok[i] = ok;
        }
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
        const int co = n0 + lrow + RPP * i;
        b_ok[i] = co < g.Cout;
        b_ptr[i] = g.w + (int64_t)(b_ok[i] ? co : 0) * taps * g.Cin + lcol;    // row 0 stands in for rows past Cout
    }

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, hh = lane >> 5;

    f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int cslabs = g.Cin / BK;
    // Split K (gridDim.z > 1, emp_conv_splitk_bn_act_nhwc): block z sums the slabs [s_lo, s_lo + S) of the taps x Cin / BK
    // slabs of the reduction and writes its partial sums, through the identity epilogue, to plane z of a workspace
    // (out + z * M * out_ps).  gridDim.z == 1: the whole reduction, as ever.
    const int S_all = taps * cslabs;
    const int s_lo = (int)((int64_t)S_all * blockIdx.z / gridDim.z);
    const int S = (int)((int64_t)S_all * (blockIdx.z + 1) / gridDim.z) - s_lo;
    const int tap0 = s_lo / cslabs, c00 = (s_lo - tap0 * cslabs) * BK;
    if (gridDim.z > 1) g.out += (int64_t)blockIdx.z * g.M * g.out_ps;
    float4 ra[MODE == 0 ? AR : 16], rb[BROWS];

    // Staging state of the NEXT slab to load: filter tap, channel offset, and per A row the source pointer of the
    // tap (rows whose tap falls outside the image, or past M, read a dummy address and are zeroed after the load:
    // no divergent branches around the loads).  Pointers are recomputed once per tap, not per slab.
    int ld_tap = tap0, ld_c0 = c00;
    const float *a_ptr[AR];
    bool a_in[AR];
    auto set_tap = [&](int tap) {
        const int ky = tap / g.KW, kx = tap - ky * g.KW;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int iy = a_iy[i] + ky * g.dil, ix = a_ix[i] + kx * g.dil;
            a_in[i] = a_ok[i] && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            a_ptr[i] = a_in[i] ? g.x + (((int64_t)a_n[i] * g.H + iy) * g.W + ix) * g.Cin + lcol : g.x + lcol;
        }
    };
    if constexpr (MODE == 0) set_tap(tap0);
    auto load_slab = [&]() {
        if constexpr (MODE == 0) {
#pragma unroll
            for (int i = 0; i < AR; ++i) ra[i] = *reinterpret_cast<const float4 *>(a_ptr[i] + ld_c0);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) ra[i * 4 + k] = *reinterpret_cast<const float4 *>(g.x + w_off[i][k] + ld_c0);
        }
#pragma unroll
        for (int i = 0; i < BROWS; ++i) rb[i] = *reinterpret_cast<const float4 *>(b_ptr[i] + (int64_t)ld_tap * g.Cin + ld_c0);
        ld_c0 += BK;
        if (ld_c0 == g.Cin) {               // block-uniform
            ld_c0 = 0;
            ++ld_tap;
            if constexpr (MODE == 0)
                if (ld_tap < taps) set_tap(ld_tap);
        }
    };
    // a_in of the slab held in ra: captured before load_slab advances the tap
    bool r_in[AR];
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            float4 v;
            if constexpr (MODE == 0) {
                v = ra[i];
                if (!r_in[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float4 d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    d[k] = ra[i * 4 + k];
                    if (!((w_mask[i] >> k) & 1u)) d[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
#define CG_COMB(p, q, sg) make_float4(__fadd_rn(p.x, __fmul_rn(sg, q.x)), __fadd_rn(p.y, __fmul_rn(sg, q.y)), \
                                      __fadd_rn(p.z, __fmul_rn(sg, q.z)), __fadd_rn(p.w, __fmul_rn(sg, q.w)))
                const float4 c0 = CG_COMB(d[0], d[1], w_sv);      // along columns, patch row a0
                const float4 c1 = CG_COMB(d[2], d[3], w_sv);      // patch row a1
                v = CG_COMB(c0, c1, w_su);                        // along rows
#undef CG_COMB
            }
            *reinterpret_cast<float4 *>(&As[buf * CG_BM * CG_LD + (lrow + RPP * i) * CG_LD + lcol]) = v;
        }
#pragma unroll
        for (int i = 0; i < BROWS; ++i) {
            float4 v = rb[i];
            if (!b_ok[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(&Bs[buf * BN * CG_LD + (lrow + RPP * i) * CG_LD + lcol]) = v;
        }
    };
#define CG_LOAD_NEXT()                                   \
    do {                                                 \
        if constexpr (MODE == 0) {                       \
            _Pragma("unroll") for (int i_ = 0; i_ < AR; ++i_) r_in[i_] = a_in[i_]; \
        }                                                \
        load_slab();                                     \
    } while (0)

    constexpr int C4 = BN / 4;                         // float4 columns of the output tile
    constexpr int RPI = CG_THREADS / C4;               // epilogue rows per iteration
    constexpr int NRE = CG_BM / RPI;                   // epilogue iterations per thread
    const int ccol = (tid % C4) * 4, crow = tid / C4;
    const int co = n0 + ccol;
    float4 rpre[RESPF ? NRE : 1];
    if constexpr (RESPF) {
#pragma unroll
        for (int it = 0; it < NRE; ++it) {
            const int64_t p = m0 + crow + it * RPI;
            rpre[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < g.M && co + 3 < g.Cout) rpre[it] = *reinterpret_cast<const float4 *>(g.res + p * g.res_ps + co);
        }
    }

    if constexpr (GLDS) {
        // ---- LDS-direct pipeline -------------------------------------------------------------------------------
        constexpr int RPW = 64 / TPR;                                   // rows one wave-load covers
        constexpr int NL = AR + BROWS;                                  // loads per thread and slab
        const int swz_ld = (BK == 16) ? ((lrow >> 2) & 3) : ((lrow >> 1) & 7);
        const int csw = (((tid % TPR) ^ swz_ld) * 4);                   // logical chunk this lane fetches (floats)
        const float *ga[AR], *gb[BROWS];
        bool ga_ok[AR];
        auto set_tap_g = [&](int tap) {
            const int ky = tap / g.KW, kx = tap - ky * g.KW;
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int iy = a_iy[i] + ky * g.dil, ix = a_ix[i] + kx * g.dil;
                ga_ok[i] = a_ok[i] && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
                ga[i] = ga_ok[i] ? g.x + (((int64_t)a_n[i] * g.H + iy) * g.W + ix) * g.Cin + csw : cg_zero_page + csw;
            }
        };
#pragma unroll
        for (int i = 0; i < BROWS; ++i) {
            const int cob = n0 + lrow + RPP * i;
            gb[i] = (cob < g.Cout) ? g.w + (int64_t)cob * taps * g.Cin + csw : cg_zero_page + csw;
        }
        set_tap_g(tap0);
        const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)smem;
        const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(RPW * wave * BK * 4));
        const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((A_ELEMS + RPW * wave * BK) * 4));
        int gl_tap = tap0, gl_c0 = c00;
        auto issue_slab = [&](int ring) {
#pragma unroll
            for (int i = 0; i < AR; ++i)
                cg_glds16(ga[i] + (ga_ok[i] ? gl_c0 : 0), a_dst + (unsigned)((ring * CG_BM + RPP * i) * BK * 4));
#pragma unroll
            for (int i = 0; i < BROWS; ++i) {
                const bool ok = n0 + lrow + RPP * i < g.Cout;
                cg_glds16(gb[i] + (ok ? (int64_t)gl_tap * g.Cin + gl_c0 : 0), b_dst + (unsigned)((ring * BN + RPP * i) * BK * 4));
            }
            gl_c0 += BK;
            if (gl_c0 == g.Cin) {               // block-uniform
                gl_c0 = 0;
                ++gl_tap;
                if (gl_tap < taps) set_tap_g(gl_tap);
            }
        };
        const int swz_rd = (BK == 16) ? ((r >> 2) & 3) : ((r >> 1) & 7);
        // Vector-memory operations in flight in this loop, in issue order (vmcnt retires in order):
        //   [RESPF only] the NRE float4 residual prefetches issued before this point (compiler-tracked loads into
        //   VGPRs; they are OLDER than every LDS-direct load, so any wait that lets at most NL younger operations
        //   stay pending has also retired them -- and the compiler inserts its own wait before their first use in the
        //   epilogue), then NL untracked LDS-direct loads per issued slab.  No stores and no atomics are issued before
        //   the K loop ends (the PROJ atomics and all output stores live in the epilogue, after the final barrier).
        //   cg_wait_vm<NL>: everything but the youngest slab's NL loads has landed; cg_wait_vm<0>: everything has.
        issue_slab(0);
        if (NBUF == 3 && S > 1) issue_slab(1);
        if (NBUF == 3 && S > 1) cg_wait_vm<NL>(); else cg_wait_vm<0>();      // slab 0 landed (slab 1 may be pending)
        __builtin_amdgcn_s_barrier();
        for (int s = 0; s < S; ++s) {
            const int ring = s % NBUF;
            if (s + NBUF - 1 < S) issue_slab((s + NBUF - 1) % NBUF);   // its buffer was read in iteration s - 1
            const float *Ar = &As[ring * CG_BM * CG_LD + (wm * 64 + r) * CG_LD];
            const float *Br = &Bs[ring * BN * CG_LD + (wn * 32 * NT + r) * CG_LD];
#pragma unroll
            for (int f = 0; f < NF4; ++f) {
                const int pc = (((hh * NF4 + f) ^ swz_rd) * 4);         // physical position of logical chunk hh*NF4 + f
                float4 fa[2], fb[NT];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4 *>(Ar + i * 32 * CG_LD + pc);
#pragma unroll
                for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const float4 *>(Br + j * 32 * CG_LD + pc);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float av[2], bv[NT];
#pragma unroll
                    for (int i = 0; i < 2; ++i) av[i] = e == 0 ? fa[i].x : e == 1 ? fa[i].y : e == 2 ? fa[i].z : fa[i].w;
#pragma unroll
                    for (int j = 0; j < NT; ++j) bv[j] = e == 0 ? fb[j].x : e == 1 ? fb[j].y : e == 2 ? fb[j].z : fb[j].w;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
                }
            }
            // slab s+1 must have landed (it was requested one or two iterations ago); the loads issued in this
            // iteration (slab s + NBUF - 1) may stay in flight when the ring has three slots
            if (NBUF == 3 && s + 2 < S) cg_wait_vm<NL>(); else cg_wait_vm<0>();
            __builtin_amdgcn_s_barrier();
        }
    } else {
        // Pipeline: slab s is consumed from LDS buffer s & 1 while slab s+1 (already in registers, loaded one
        // iteration earlier) is written to the other buffer between the MFMAs, and the global loads of slab s+2 are
        // issued right behind it: a load has a whole iteration (64 MFMAs per wave) to land, and the LDS writes, address
        // arithmetic and load issue all overlap the matrix pipe.
        CG_LOAD_NEXT();
        store_slab(0);
        if (S > 1) CG_LOAD_NEXT();
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const int buf = s & 1;
            const float *Ab = &As[buf * CG_BM * CG_LD + (wm * 64 + r) * CG_LD + hh * (BK / 2)];
            const float *Bb = &Bs[buf * BN * CG_LD + (wn * 32 * NT + r) * CG_LD + hh * (BK / 2)];
    #pragma unroll
            for (int half = 0; half < NF4 / 2; ++half) {
                float4 fa[2][2], fb[NT][2];
    #pragma unroll
                for (int q = 0; q < 2; ++q) {
    #pragma unroll
                    for (int i = 0; i < 2; ++i)
                        fa[i][q] = *reinterpret_cast<const float4 *>(Ab + i * 32 * CG_LD + half * 8 + q * 4);
    #pragma unroll
                    for (int j = 0; j < NT; ++j)
                        fb[j][q] = *reinterpret_cast<const float4 *>(Bb + j * 32 * CG_LD + half * 8 + q * 4);
                }
    #pragma unroll
                for (int q = 0; q < 2; ++q) {
    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float av[2], bv[NT];
    #pragma unroll
                        for (int i = 0; i < 2; ++i)
                            av[i] = e == 0 ? fa[i][q].x : e == 1 ? fa[i][q].y : e == 2 ? fa[i][q].z : fa[i][q].w;
    #pragma unroll
                        for (int j = 0; j < NT; ++j)
                            bv[j] = e == 0 ? fb[j][q].x : e == 1 ? fb[j][q].y : e == 2 ? fb[j][q].z : fb[j][q].w;
    #pragma unroll
                        for (int i = 0; i < 2; ++i)
    #pragma unroll
                            for (int j = 0; j < NT; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
                    }
                    if (half == 0 && q == 0) {
                        if (s + 1 < S) store_slab(buf ^ 1);     // slab s+1: registers -> the buffer read in iteration s-1
                        if (s + 2 < S) CG_LOAD_NEXT();          // slab s+2: global -> registers
                    }
                }
            }
            __syncthreads();
        }

    }

    // epilogue, staged through LDS so that global traffic is 16 bytes per lane and row-contiguous:
    // accumulators -> LDS tile [EPI_ROWS][BN] (C/D map: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)),
    // then y = relu?(acc * scale[co] + shift[co] (+ residual)) written as float4 along cout.  With the small-LDS
    // variant the tile is staged in two rounds of 64 rows (the rows of the waves wm = 0, then wm = 1).
    float *Cs = smem;                                  // the K loop ended with a barrier: As / Bs are free
    const bool vec_ok = (co + 3 < g.Cout) && ((g.out_ps & 3) == 0) && ((g.res_ps & 3) == 0) &&
                        ((reinterpret_cast<uintptr_t>(g.out) & 15) == 0) &&
                        (!g.res || (reinterpret_cast<uintptr_t>(g.res) & 15) == 0) && ((g.Cout & 3) == 0);
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (co + e < g.Cout) {
            if (g.scale) sc[e] = g.scale[co + e];
            if (g.shift) sh[e] = g.shift[co + e];
        }
    constexpr int ROUNDS = CG_BM / EPI_ROWS;
    constexpr int NRR = EPI_ROWS / RPI;                // epilogue iterations per thread and round
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        if (rd > 0) __syncthreads();                   // the previous round's reads are done
        if (ROUNDS == 1 || wm == rd) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = (ROUNDS == 1 ? wm * 64 : 0) + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
                        Cs[row * CLD + wn * 32 * NT + j * 32 + r] = acc[i][j][q];
                    }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NRR; ++it) {
            const int lrow_c = crow + it * RPI;            // row inside the staged chunk
            const int row = rd * EPI_ROWS + lrow_c;        // row inside the block tile
            const int64_t p = m0 + row;
            const bool valid = p < g.M;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (valid) {
                const float4 a4 = *reinterpret_cast<const float4 *>(&Cs[lrow_c * CLD + ccol]);
                v[0] = a4.x; v[1] = a4.y; v[2] = a4.z; v[3] = a4.w;
                float rr[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (RESPF) {
                    const float4 r4 = rpre[rd * NRR + it];
                    rr[0] = r4.x; rr[1] = r4.y; rr[2] = r4.z; rr[3] = r4.w;
                } else if (g.res) {
                    if (vec_ok) {
                        const float4 r4 = *reinterpret_cast<const float4 *>(g.res + p * g.res_ps + co);
                        rr[0] = r4.x; rr[1] = r4.y; rr[2] = r4.z; rr[3] = r4.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < g.Cout) rr[e] = g.res[p * g.res_ps + co + e];
                    }
                }
                if (RESPF && g.scale && g.shift) {          // the common case of the prefetch variant, straight-line
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(__fadd_rn(__fmul_rn(v[e], sc[e]), sh[e]), rr[e]);
                    if (g.relu) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                } else if (!RESPF && !GATE && !g.res && g.scale && g.shift) {   // BN (+ ReLU) only
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(__fmul_rn(v[e], sc[e]), sh[e]);
                    if (g.relu) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                } else
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (g.scale) v[e] = __fmul_rn(v[e], sc[e]);
                    if (g.shift) v[e] = __fadd_rn(v[e], sh[e]);
                    if constexpr (GATE) {                   // squeeze-excite gate: res * sigmoid(v)
                        v[e] = __fmul_rn(rr[e], __fdiv_rn(1.f, __fadd_rn(1.f, expf(-v[e]))));
                    } else {
                        if (g.res) v[e] = __fadd_rn(v[e], rr[e]);
                        if (g.relu) v[e] = fmaxf(v[e], 0.f);
                    }
                }
                if (!PROJ || g.out) {
                    if (vec_ok) {
                        *reinterpret_cast<float4 *>(g.out + p * g.out_ps + co) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < g.Cout) g.out[p * g.out_ps + co + e] = v[e];
                    }
                }
            }
            if constexpr (PROJ) {
                // lane partials of the following 1x1 convolution, parked in the thread's own (already consumed)
                // float4 slot of the staging tile: component q = output channel q
                float ps[4] = {0.f, 0.f, 0.f, 0.f};
                if (valid && co + 3 < g.Cout) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < g.proj_n) {
                            const float4 wq = *reinterpret_cast<const float4 *>(g.proj_w + (int64_t)q * g.Cout + co);
                            ps[q] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], wq.x), __fmul_rn(v[1], wq.y)),
                                                        __fmul_rn(v[2], wq.z)), __fmul_rn(v[3], wq.w));
                        }
                }
                *reinterpret_cast<float4 *>(&Cs[lrow_c * CLD + ccol]) = make_float4(ps[0], ps[1], ps[2], ps[3]);
            }
        }
        if constexpr (PROJ) {
            __syncthreads();
            for (int idx = tid; idx < EPI_ROWS * g.proj_n; idx += CG_THREADS) {
                const int row_l = idx / g.proj_n, q = idx - row_l * g.proj_n;
                const int64_t p = m0 + rd * EPI_ROWS + row_l;
                if (p < g.M) {
                    float t = Cs[row_l * CLD + q];
#pragma unroll 8
                    for (int j = 1; j < C4; ++j) t = __fadd_rn(t, Cs[row_l * CLD + 4 * j + q]);   // lanes in ascending order
                    const int64_t img = p / g.hw;
                    atomicAdd(g.proj_out + (img * g.proj_n + q) * g.hw + (p - img * g.hw), t);
                }
            }
        }
    }
}

// Tile / K-slab selection, shared by the launchers and exported so that the oracle can mirror the summation order.
// 16-wide slabs (three resident blocks per CU instead of two: each block's prologue / epilogue hides behind the
// matrix work of two others) unless the launch has at most two blocks per CU anyway, or the residual-prefetch
// variant is used (it needs the registers).
struct CgPlan {
    bool narrow, respf, glds;
    int slab, tiles_m, tiles_n;
};

static CgPlan cg_plan(int64_t M, int Cout, int batch, bool has_res, bool res_vec_ok, bool may_split_n = true, int cin = 32)
{
    CgPlan p;
    // 64-wide cout tiles for narrow layers, and whenever 128-wide tiles would leave CUs without a block (small
    // launches: the per-slice protocol at batch 1 has 8-64 pixel tiles in layer3 / layer4).  The K order, hence the
    // summation order, does not depend on the cout tiling.
    const int64_t wide_blocks = emp_cdiv(M, CG_BM) * emp_cdiv(Cout, 128) * batch;
    p.narrow = Cout <= 64 || (Cout % 128 != 0 && Cout % 128 <= 64 && Cout < 512) || (may_split_n && wide_blocks < 256);
    p.tiles_m = (int)emp_cdiv(M, CG_BM);
    p.tiles_n = (int)emp_cdiv(Cout, p.narrow ? 64 : 128);
    static const char *fnarrow = getenv("EMP_CONV_NARROW");    // experiments only: "1" forces 64-wide cout tiles
    static const char *norespf = getenv("EMP_CONV_NO_RESPF");  // experiments only
    if (fnarrow && fnarrow[0] == '1') {
        p.narrow = true;
        p.tiles_n = (int)emp_cdiv(Cout, 64);
    }
    p.respf = has_res && res_vec_ok && Cout % (p.narrow ? 64 : 128) == 0 && !norespf;
    static const char *force = getenv("EMP_CONV_BK");          // experiments only: "16" / "32"
    const int64_t blocks = (int64_t)p.tiles_m * p.tiles_n * batch;
    p.slab = blocks > 512 ? 16 : 32;
    if (force && force[0] == '1') p.slab = 16;
    if (force && force[0] == '3') p.slab = 32;
    if (p.respf) p.slab = 32;
    if (cin % 32 != 0) {                 // Cin a multiple of 16 only (RegNet widths 144, 1296): 16-wide slabs throughout
        p.slab = 16;
        p.respf = false;
    }
    static const char *noglds = getenv("EMP_CONV_NO_GLDS");          // experiments only
    p.glds = !noglds;
    return p;
}

extern "C" int emp_conv_k_slab(int64_t M, int Cout, int batch, int has_residual)
{
    return cg_plan(M, Cout, batch, has_residual != 0, true).slab;
}

extern "C" int emp_conv_k_slab_cin(int64_t M, int Cout, int batch, int has_residual, int Cin)
{
    return cg_plan(M, Cout, batch, has_residual != 0, true, true, Cin).slab;
}

// D4b (emp_conv1x1.hip): the weight-stationary kernel for short-K pointwise layers.  Kind 1 (conv3 / shortcut shapes) sums
// over 64-channel slabs; kind 2 (256 -> 64, 64 -> 64, 256 -> 128 without a residual) and the batched GEMM sum in the
// order of the tiled kernel's plan, so emp_conv_k_slab* keep their answers for them; so does kind 3 (Cin 256 + residual:
// layer3's conv3), in the 32-channel slabs of the residual-prefetch plan.
extern "C" __attribute__((visibility("hidden"))) int emp_conv1x1_ws_kind(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int has_residual);
extern "C" __attribute__((visibility("hidden"))) int emp_conv1x1_ws_launch(int kind, const float *x, const float *w, const float *scale, const float *shift,
                                     const float *res, int64_t res_ps, int relu, int64_t M, int Cin, int Cout,
                                     float *out, int64_t out_ps, void *stream);
extern "C" __attribute__((visibility("hidden"))) int emp_gemm_ws_eligible(int batch, int64_t M, int N, int K, int slab);
extern "C" __attribute__((visibility("hidden"))) int emp_gemm_ws_launch(const float *A, const float *B, int batch, int64_t M, int N, int K, float *C,
                                                                        void *stream);

// D4c (emp_conv_stream.hip): the persistent tile-stream form of the tiled kernel for its GEMM-shaped launches -- 1x1,
// stride 1, no padding, no residual, relu in {0, 1}, Cout a multiple of 128, and a plan that says K-slab 16, LDS-direct,
// 128-wide tiles -- from CS_MIN_TOTAL tiles on (8/3 for each of the 768 resident blocks: the smallest launches measured,
// profiles/conv_stream.md).  Same summation order, same epilogue arithmetic: emp_conv_k_slab* keep their answers.  The
// weight-stationary kernels keep their shapes: the launchers ask this after them, and the query answers 0 for a
// geometry emp_conv1x1_ws_kind / emp_gemm_ws_eligible name.
// proj != 0 (emp_conv_bn_act_proj_nhwc): not built, always 0.  EMP_CONV_NO_STREAM=1: experiments only, forces the
// one-tile-per-block kernel; EMP_CONV_STREAM_MIN_TILES=n: experiments only, the minimum becomes n tiles per block.
#define CS_MIN_TOTAL 2048
extern "C" __attribute__((visibility("hidden"))) int emp_conv_stream_launch(const float *x, const float *w, const float *scale, const float *shift,
                                                                            int relu, int batch, int64_t M, int Cin, int Cout,
                                                                            int64_t x_bs, int64_t w_bs, int64_t out_bs, float *out,
                                                                            int64_t out_ps, void *stream);
extern "C" int emp_conv_stream_grid(int64_t tiles, int batch);

extern "C" int emp_conv_stream_eligible(int batch, int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                                        int has_residual, int proj)
{
    static const char *off = getenv("EMP_CONV_NO_STREAM");
    const char *mint = getenv("EMP_CONV_STREAM_MIN_TILES");    // read per call: tests set it for single launches
    if (off && off[0] == '1') return 0;
    if (proj || has_residual || batch < 1 || M <= 0 || Cin <= 0 || Cout <= 0) return 0;
    if (!(KH == 1 && KW == 1 && stride == 1 && pad == 0 && (relu == 0 || relu == 1))) return 0;
    if (Cout % 128 != 0 || Cin % 16 != 0) return 0;
    CgPlan pl;
    if (batch > 1) {                                   // emp_gemm_nt_batched
        if (Cin % CG_BK != 0) return 0;
        pl = cg_plan(M, Cout, batch, false, true);
        if (emp_gemm_ws_eligible(batch, M, Cout, Cin, pl.slab)) return 0;
    } else {
        pl = cg_plan(M, Cout, 1, false, true, true, Cin);
        if (emp_conv1x1_ws_kind(M, Cin, Cout, KH, KW, stride, pad, relu, 0) != 0) return 0;
    }
    if (!(pl.slab == 16 && pl.glds && !pl.narrow && !pl.respf)) return 0;
    const int64_t total = (int64_t)pl.tiles_m * pl.tiles_n * batch;
    const int64_t min_total = mint ? atoll(mint) * emp_conv_stream_grid(total, 1) : CS_MIN_TOTAL;
    if (total >= (1LL << 28) || total < min_total) return 0;
    return 1;
}

extern "C" int emp_conv_k_slab_geom(int64_t M, int Cout, int has_residual, int Cin, int KH, int KW, int stride, int pad,
                                    int relu)
{
    if (emp_conv1x1_ws_kind(M, Cin, Cout, KH, KW, stride, pad, relu, has_residual) == 1) return 64;
    return cg_plan(M, Cout, 1, has_residual != 0 && relu != 2, true, true, Cin).slab;
}

extern "C" int emp_conv_bn_act_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                                    const float *residual, int64_t res_pixel_stride, int relu, int N, int H, int W,
                                    int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, float *out,
                                    int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(x && w_okkc && out, "conv: null pointer");
    EMP_REQUIRE(N >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv: bad shape");
    EMP_REQUIRE(Cin % 16 == 0, "conv: Cin %d must be a multiple of 16", Cin);
    EMP_REQUIRE(relu != 2 || residual, "conv: the gate epilogue (relu == 2) needs the gated tensor as residual");
    EMP_REQUIRE(KH >= 1 && KW >= 1 && KH <= 7 && KW <= 7 && stride >= 1 && dil >= 1 && pad >= 0, "conv: bad filter geometry");
    const int OH = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    const int OW = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    EMP_REQUIRE(OH > 0 && OW > 0, "conv: empty output");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    if (res_pixel_stride == 0) res_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout && res_pixel_stride >= Cout, "conv: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_okkc)) & 15) == 0,
                "conv: x and w must be 16-byte aligned");
    EMP_REQUIRE(out != x, "conv: output cannot alias the input");
    if (N == 0) return EMP_OK;
    ConvGeom g;
    g.x = x; g.w = w_okkc; g.scale = scale; g.shift = shift; g.res = residual; g.out = out;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.OH = OH; g.OW = OW; g.Cout = Cout; g.KH = KH; g.KW = KW;
    g.stride = stride; g.pad = pad; g.dil = dil; g.relu = relu;
    g.M = (int64_t)N * OH * OW; g.out_ps = out_pixel_stride; g.res_ps = res_pixel_stride;
    g.x_bs = g.w_bs = g.out_bs = 0; g.tiles = nullptr; g.proj_w = nullptr; g.proj_out = nullptr; g.proj_n = 0; g.hw = 1;
    const bool res_vec_ok = (res_pixel_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(residual) & 15) == 0;
    const bool io_vec_ok = res_vec_ok && (out_pixel_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                           (!scale || (reinterpret_cast<uintptr_t>(scale) & 15) == 0) &&
                           (!shift || (reinterpret_cast<uintptr_t>(shift) & 15) == 0);
    const int ws = io_vec_ok && scale && shift ? emp_conv1x1_ws_kind(g.M, Cin, Cout, KH, KW, stride, pad, relu, residual != nullptr) : 0;
    if (ws == 1)
        return emp_conv1x1_ws_launch(1, x, w_okkc, scale, shift, residual, res_pixel_stride, relu, g.M, Cin, Cout, out,
                                     out_pixel_stride, stream);
    const CgPlan pl = cg_plan(g.M, Cout, 1, residual != nullptr && relu != 2, res_vec_ok, true, Cin);
    if (ws == 2 && !residual && pl.slab == 16)       // same summation order as the tiled kernel below
        return emp_conv1x1_ws_launch(2, x, w_okkc, scale, shift, nullptr, res_pixel_stride, relu, g.M, Cin, Cout, out,
                                     out_pixel_stride, stream);
    if (ws == 3 && residual && pl.respf && pl.slab == 32 &&  // likewise: the residual-prefetch plan's 32-channel slabs
        res_pixel_stride < (1 << 24) && out_pixel_stride < (1 << 24))   // (its lane offsets are 32-bit)
        return emp_conv1x1_ws_launch(3, x, w_okkc, scale, shift, residual, res_pixel_stride, relu, g.M, Cin, Cout, out,
                                     out_pixel_stride, stream);
    if (io_vec_ok && scale && shift && !residual &&
        emp_conv_stream_eligible(1, g.M, Cin, Cout, KH, KW, stride, pad, relu, 0, 0))
        return emp_conv_stream_launch(x, w_okkc, scale, shift, relu, 1, g.M, Cin, Cout, 0, 0, 0, out, out_pixel_stride, stream);
    const bool narrow = pl.narrow, respf = pl.respf, bk16 = pl.slab == 16;
    EMP_REQUIRE((int64_t)pl.tiles_m * pl.tiles_n < (1LL << 28), "conv: too many tiles");
    g.tiles_m = pl.tiles_m;
    g.tiles_n = pl.tiles_n;
    const int T = g.tiles_m * g.tiles_n;
    const int grid = 8 * ((T + 7) / 8);
#define CG_GO(NT_, RES_, BK_, GL_) hipLaunchKernelGGL((conv_igemm_f32_kernel<NT_, 0, RES_, BK_, false, GL_>), dim3(grid), dim3(CG_THREADS), 0, emp_stream(stream), g)
#define CG_GATE(NT_, BK_) hipLaunchKernelGGL((conv_igemm_f32_kernel<NT_, 0, false, BK_, false, true, true>), dim3(grid), dim3(CG_THREADS), 0, emp_stream(stream), g)
    if (relu == 2) {                         // gate epilogue: LDS-direct staging, residual read in the epilogue
        if (narrow) { if (bk16) CG_GATE(1, 16); else CG_GATE(1, 32); }
        else { if (bk16) CG_GATE(2, 16); else CG_GATE(2, 32); }
    } else if (narrow) {
        if (respf) { if (pl.glds) CG_GO(1, true, 32, true); else CG_GO(1, true, 32, false); }
        else if (pl.glds) { if (bk16) CG_GO(1, false, 16, true); else CG_GO(1, false, 32, true); }
        else { if (bk16) CG_GO(1, false, 16, false); else CG_GO(1, false, 32, false); }
    } else {
        if (respf) { if (pl.glds) CG_GO(2, true, 32, true); else CG_GO(2, true, 32, false); }
        else if (pl.glds) { if (bk16) CG_GO(2, false, 16, true); else CG_GO(2, false, 32, true); }
        else { if (bk16) CG_GO(2, false, 16, false); else CG_GO(2, false, 32, false); }
    }
#undef CG_GO
#undef CG_GATE
    EMP_CHECK_LAUNCH("emp_conv_bn_act_nhwc");
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------
// Split-K form for SMALL launches (a 512^2 tile at batch 1 leaves layer3 / layer4 / ASPP with 8-64 tiles of 128 pixels
// on 256 CUs: profiles/r3_batch1_forward_512.md).  The reduction is cut into k_splits ranges of whole 32-channel slabs,
// every range is a block of its own (gridDim.z) that writes its partial sums to a workspace, and a second pass adds the
// partials in ascending order and applies the epilogue:
//   out = relu?((((p_0 + p_1) + p_2) + ...) * scale + shift (+ residual)),  p_z = the fmaf chain of emp_conv_bn_act_nhwc
//   (K-slab 32) over slabs [S z / k, S (z + 1) / k) of the S = KH KW Cin / 32 slabs, from +0.
// Deterministic (no atomics); oracle/dense.py::conv_bn_act_nhwc(slab=32, k_splits=k) restates it.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float *__restrict__ work, int nz, int64_t M, int Cout,
                                                            const float *__restrict__ scale,
                                                            const float *__restrict__ shift,
                                                            const float *__restrict__ res, int64_t res_ps, int relu,
                                                            float *__restrict__ out, int64_t out_ps)
{
    const int C4 = Cout >> 2;
    const int64_t total = M * C4, plane = M * (int64_t)Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / C4;
        const int co = (int)(i - p * C4) * 4;
        const float *w = work + p * Cout + co;
        float4 t = *reinterpret_cast<const float4 *>(w);
        for (int z = 1; z < nz; ++z) {
            const float4 u = *reinterpret_cast<const float4 *>(w + z * plane);
            t.x = __fadd_rn(t.x, u.x); t.y = __fadd_rn(t.y, u.y); t.z = __fadd_rn(t.z, u.z); t.w = __fadd_rn(t.w, u.w);
        }
        float v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sc = scale ? scale[co + e] : 1.f, sh = shift ? shift[co + e] : 0.f;
            v[e] = __fadd_rn(__fmul_rn(v[e], sc), sh);
        }
        if (res) {
            const float4 r4 = *reinterpret_cast<const float4 *>(res + p * res_ps + co);
            v[0] = __fadd_rn(v[0], r4.x); v[1] = __fadd_rn(v[1], r4.y); v[2] = __fadd_rn(v[2], r4.z); v[3] = __fadd_rn(v[3], r4.w);
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        *reinterpret_cast<float4 *>(out + p * out_ps + co) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// how many ranges a launch of this geometry should be cut into (1: it fills the chip as it is, or cannot be cut)
extern "C" int emp_conv_splitk_plan(int64_t M, int Cout, int Cin, int KH, int KW)
{
    if (M <= 0 || Cout <= 0 || Cin % 32 != 0 || Cout % 4 != 0) return 1;
    const CgPlan pl = cg_plan(M, Cout, 1, false, true, true, Cin);
    const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n;
    const int S = KH * KW * (Cin / 32);
    // A block's life is ~6 us of prologue + epilogue plus 0.85 us of matrix work per slab (one wave per SIMD, two
    // accumulator chains: the matrix pipe of its CU is busy), so the launch is as fast as its LONGEST ROUND of blocks:
    // cut until the blocks just fill the 256 CUs once (tiles 32, S 72: 8 ranges, 256 blocks, 14 us; 10 ranges -- 320
    // blocks, two rounds -- measured 25 us)
    if (tiles > 128) return 1;
    int64_t k = 256 / tiles;
    if (k > S / 4) k = S / 4;                       // at least four slabs per range
    if (k > 32) k = 32;
    return k >= 2 ? (int)k : 1;
}

extern "C" int emp_conv_splitk_bn_act_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                                           const float *residual, int64_t res_pixel_stride, int relu, int N, int H, int W,
                                           int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int k_splits,
                                           float *work, float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(x && w_okkc && out && work, "conv_splitk: null pointer");
    EMP_REQUIRE(N >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv_splitk: bad shape");
    EMP_REQUIRE(Cin % 32 == 0 && Cout % 4 == 0, "conv_splitk: Cin %d must be a multiple of 32, Cout %d of 4", Cin, Cout);
    EMP_REQUIRE(relu == 0 || relu == 1, "conv_splitk: relu must be 0 or 1");
    EMP_REQUIRE(KH >= 1 && KW >= 1 && KH <= 7 && KW <= 7 && stride >= 1 && dil >= 1 && pad >= 0, "conv_splitk: bad filter geometry");
    const int OH = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    const int OW = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    EMP_REQUIRE(OH > 0 && OW > 0, "conv_splitk: empty output");
    const int S = KH * KW * (Cin / 32);
    EMP_REQUIRE(k_splits >= 1 && k_splits <= S && k_splits <= 64, "conv_splitk: k_splits %d not in 1..min(%d, 64)", k_splits, S);
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    if (res_pixel_stride == 0) res_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout && res_pixel_stride >= Cout, "conv_splitk: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_okkc) | reinterpret_cast<uintptr_t>(work) |
                  reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(scale) |
                  reinterpret_cast<uintptr_t>(shift)) & 15) == 0 && (out_pixel_stride & 3) == 0 && (res_pixel_stride & 3) == 0,
                "conv_splitk: pointers must be 16-byte aligned, pixel strides multiples of 4");
    EMP_REQUIRE(out != x && work != x && work != out, "conv_splitk: buffers must not alias");
    if (N == 0) return EMP_OK;
    ConvGeom g;
    g.x = x; g.w = w_okkc; g.scale = nullptr; g.shift = nullptr; g.res = nullptr; g.out = work;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.OH = OH; g.OW = OW; g.Cout = Cout; g.KH = KH; g.KW = KW;
    g.stride = stride; g.pad = pad; g.dil = dil; g.relu = 0;
    g.M = (int64_t)N * OH * OW; g.out_ps = Cout; g.res_ps = Cout;
    g.x_bs = g.w_bs = g.out_bs = 0; g.tiles = nullptr; g.proj_w = nullptr; g.proj_out = nullptr; g.proj_n = 0; g.hw = 1;
    const CgPlan pl = cg_plan(g.M, Cout, 1, false, true, true, Cin);
    EMP_REQUIRE((int64_t)pl.tiles_m * pl.tiles_n < (1LL << 28), "conv_splitk: too many tiles");
    g.tiles_m = pl.tiles_m;
    g.tiles_n = pl.tiles_n;
    const int T = g.tiles_m * g.tiles_n;
    const dim3 grid(8 * ((T + 7) / 8), 1, k_splits);
    hipStream_t st = emp_stream(stream);
    if (pl.narrow)
        hipLaunchKernelGGL((conv_igemm_f32_kernel<1, 0, false, 32, false, true>), grid, dim3(CG_THREADS), 0, st, g);
    else
        hipLaunchKernelGGL((conv_igemm_f32_kernel<2, 0, false, 32, false, true>), grid, dim3(CG_THREADS), 0, st, g);
    EMP_CHECK_LAUNCH("emp_conv_splitk_bn_act_nhwc(partials)");
    const int64_t total = g.M * (Cout / 4);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(emp_grid(total, 256, 4096)), dim3(256), 0, st, work, k_splits, g.M, Cout,
                       scale, shift, residual, res_pixel_stride, relu, out, out_pixel_stride);
    EMP_CHECK_LAUNCH("emp_conv_splitk_bn_act_nhwc(reduce)");
    return EMP_OK;
}

extern "C" int emp_conv_bn_act_proj_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                                         int relu, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                         int pad, int dil, const float *proj_w, int proj_n, float *proj_out,
                                         float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(x && w_okkc && proj_w && proj_out, "conv_proj: null pointer");
    EMP_REQUIRE(N >= 0 && H > 0 && W > 0 && Cin > 0 && Cin % CG_BK == 0, "conv_proj: bad shape (Cin %% %d)", CG_BK);
    EMP_REQUIRE(Cout == 128 || Cout == 256, "conv_proj: Cout %d must be 128 or 256 (at most two cout tiles)", Cout);
    EMP_REQUIRE(proj_n >= 1 && proj_n <= 4, "conv_proj: proj_n %d not in 1..4", proj_n);
    EMP_REQUIRE(KH >= 1 && KW >= 1 && KH <= 7 && KW <= 7 && stride >= 1 && dil >= 1 && pad >= 0, "conv_proj: bad filter geometry");
    const int OH = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    const int OW = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    EMP_REQUIRE(OH > 0 && OW > 0, "conv_proj: empty output");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_okkc) | reinterpret_cast<uintptr_t>(proj_w) |
                  reinterpret_cast<uintptr_t>(out)) & 15) == 0 && (out_pixel_stride & 3) == 0, "conv_proj: alignment");
    EMP_REQUIRE(out != x, "conv_proj: output cannot alias the input");
    if (N == 0) return EMP_OK;
    ConvGeom g;
    g.x = x; g.w = w_okkc; g.scale = scale; g.shift = shift; g.res = nullptr; g.out = out;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.OH = OH; g.OW = OW; g.Cout = Cout; g.KH = KH; g.KW = KW;
    g.stride = stride; g.pad = pad; g.dil = dil; g.relu = relu;
    g.M = (int64_t)N * OH * OW; g.out_ps = out_pixel_stride; g.res_ps = Cout;
    g.x_bs = g.w_bs = g.out_bs = 0; g.tiles = nullptr;
    g.proj_w = proj_w; g.proj_out = proj_out; g.proj_n = proj_n; g.hw = (int64_t)OH * OW;
    const CgPlan pl = cg_plan(g.M, Cout, 1, false, true, false);      // the fold needs whole 128-wide cout tiles
    g.tiles_m = pl.tiles_m;
    g.tiles_n = pl.tiles_n;
    const int T = g.tiles_m * g.tiles_n;
    const int grid = 8 * ((T + 7) / 8);
#define CG_GOP(BK_, GL_) hipLaunchKernelGGL((conv_igemm_f32_kernel<2, 0, false, BK_, true, GL_>), dim3(grid), dim3(CG_THREADS), 0, emp_stream(stream), g)
    if (pl.glds) { if (pl.slab == 16) CG_GOP(16, true); else CG_GOP(32, true); }
    else { if (pl.slab == 16) CG_GOP(16, false); else CG_GOP(32, false); }
#undef CG_GOP
    EMP_CHECK_LAUNCH("emp_conv_bn_act_proj_nhwc");
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------
// D5: Winograd F(2x2, 3x3) for the 3x3 (dilated) stride-1 "same" convolutions with many input channels (ASPP,
// layer4): 2.25x fewer matrix-core FLOPs than the direct form.  A dilated convolution is d*d independent plain
// 3x3 convolutions on the sub-grids (y mod d, x mod d); each 2x2 output tile of a sub-grid needs a 4x4 input patch
// with pixel spacing d.  Three steps: input transform V = B^T d B (this file), 16 GEMMs M_p = V_p U_p^T on the
// fp32 matrix cores (conv_igemm_f32_kernel, blockIdx.y = position p), output transform Y = A^T M A fused with the
// BatchNorm / ReLU epilogue.  tiles: (T, 3) int32 = (image n, y, x of the patch's top-left pixel), built by the host.

// x (N,H,W,C) -> V (16, T, C); one thread per (tile, 4 channels)
__global__ __launch_bounds__(256) void wino_input_kernel(const float *__restrict__ x, const int32_t *__restrict__ tiles,
                                                         int64_t T, int H, int W, int C4, int dil, float4 *__restrict__ V)
{
    const int64_t total = T * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const int64_t t = i / C4;
        const int n = tiles[3 * t], by = tiles[3 * t + 1], bx = tiles[3 * t + 2];
        const float4 *src = reinterpret_cast<const float4 *>(x) + (int64_t)n * H * W * C4 + c4;
        float4 d[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int yy = by + a * dil, xx = bx + b * dil;
                d[a][b] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) d[a][b] = src[((int64_t)yy * W + xx) * C4];
            }
#define W_SUB(p, q) make_float4(__fsub_rn(p.x, q.x), __fsub_rn(p.y, q.y), __fsub_rn(p.z, q.z), __fsub_rn(p.w, q.w))
#define W_ADD(p, q) make_float4(__fadd_rn(p.x, q.x), __fadd_rn(p.y, q.y), __fadd_rn(p.z, q.z), __fadd_rn(p.w, q.w))
        float4 tt[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {          // along columns: t[a] = d[a] B
            tt[a][0] = W_SUB(d[a][0], d[a][2]);
            tt[a][1] = W_ADD(d[a][1], d[a][2]);
            tt[a][2] = W_SUB(d[a][2], d[a][1]);
            tt[a][3] = W_SUB(d[a][1], d[a][3]);
        }
        float4 *dst = V + t * C4 + c4;
        const int64_t ps = T * C4;             // position stride
#pragma unroll
        for (int v = 0; v < 4; ++v) {          // along rows: V = B^T t
            dst[(0 * 4 + v) * ps] = W_SUB(tt[0][v], tt[2][v]);
            dst[(1 * 4 + v) * ps] = W_ADD(tt[1][v], tt[2][v]);
            dst[(2 * 4 + v) * ps] = W_SUB(tt[2][v], tt[1][v]);
            dst[(3 * 4 + v) * ps] = W_SUB(tt[1][v], tt[3][v]);
        }
    }
}

// Mw (16, T, Cout) -> out (N,H,W,Cout) with the fused epilogue; one thread per (tile, 4 couts)
__global__ __launch_bounds__(256) void wino_output_kernel(const float4 *__restrict__ Mw, const int32_t *__restrict__ tiles,
                                                          int64_t T, int H, int W, int Co4, int dil,
                                                          const float4 *__restrict__ scale, const float4 *__restrict__ shift,
                                                          int relu, float *__restrict__ out, int64_t out_ps)
{
    const int64_t total = T * Co4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % Co4);
        const int64_t t = i / Co4;
        const int n = tiles[3 * t], oy = tiles[3 * t + 1] + dil, ox = tiles[3 * t + 2] + dil;
        const float4 *src = Mw + t * Co4 + c4;
        const int64_t ps = T * Co4;
        float4 m[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) m[a][b] = src[(a * 4 + b) * ps];
        float4 s[2][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {          // rows: s = A^T m
            s[0][b] = W_ADD(W_ADD(m[0][b], m[1][b]), m[2][b]);
            s[1][b] = W_SUB(W_SUB(m[1][b], m[2][b]), m[3][b]);
        }
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (scale) sc = scale[c4];
        if (shift) sh = shift[c4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float4 yv[2];
            yv[0] = W_ADD(W_ADD(s[a][0], s[a][1]), s[a][2]);      // columns: y = s A
            yv[1] = W_SUB(W_SUB(s[a][1], s[a][2]), s[a][3]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int yy = oy + a * dil, xx = ox + b * dil;
                if (yy < H && xx < W) {
                    float4 v = yv[b];
                    if (scale) v = make_float4(__fmul_rn(v.x, sc.x), __fmul_rn(v.y, sc.y), __fmul_rn(v.z, sc.z), __fmul_rn(v.w, sc.w));
                    if (shift) v = W_ADD(v, sh);
                    if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
                    *reinterpret_cast<float4 *>(out + (((int64_t)n * H + yy) * W + xx) * out_ps + 4 * c4) = v;
                }
            }
        }
    }
}
#undef W_SUB
#undef W_ADD

extern "C" int emp_wino_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                                        int64_t T, float *V, void *stream)
{
    EMP_REQUIRE(x && tiles && V, "wino_input: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && dil >= 1 && T >= 0, "wino_input: bad shape");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(V)) & 15) == 0, "wino_input: alignment");
    if (T == 0) return EMP_OK;
    hipLaunchKernelGGL(wino_input_kernel, dim3(emp_grid(T * (C / 4), 256, 16384)), dim3(256), 0, emp_stream(stream), x,
                       tiles, T, H, W, C / 4, dil, reinterpret_cast<float4 *>(V));
    EMP_CHECK_LAUNCH("emp_wino_input_transform");
    return EMP_OK;
}

extern "C" int emp_gemm_nt_batched(const float *A, const float *B, int batch, int64_t M, int N, int K, float *C,
                                   void *stream)
{
    EMP_REQUIRE(A && B && C, "gemm: null pointer");
    EMP_REQUIRE(batch >= 1 && batch <= 65535 && M >= 0 && M < (1LL << 31) && N > 0 && K > 0 && K % CG_BK == 0,
                "gemm: bad shape (K must be a multiple of %d)", CG_BK);
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0, "gemm: alignment");
    if (M == 0) return EMP_OK;
    ConvGeom g;
    g.x = A; g.w = B; g.scale = g.shift = g.res = nullptr; g.out = C;
    g.N = 1; g.H = 1; g.W = (int)M; g.Cin = K; g.OH = 1; g.OW = (int)M; g.Cout = N; g.KH = g.KW = 1;
    g.stride = 1; g.pad = 0; g.dil = 1; g.relu = 0;
    g.M = M; g.out_ps = N; g.res_ps = N;
    g.x_bs = M * K; g.w_bs = (int64_t)N * K; g.out_bs = M * N; g.tiles = nullptr; g.proj_w = nullptr; g.proj_out = nullptr; g.proj_n = 0; g.hw = 1;
    const CgPlan pl = cg_plan(M, N, batch, false, true);
    if ((reinterpret_cast<uintptr_t>(C) & 15) == 0 && emp_gemm_ws_eligible(batch, M, N, K, pl.slab))
        return emp_gemm_ws_launch(A, B, batch, M, N, K, C, stream);       // short K: weight-stationary, same order
    if ((reinterpret_cast<uintptr_t>(C) & 15) == 0 && emp_conv_stream_eligible(batch, M, K, N, 1, 1, 1, 0, 0, 0, 0))
        return emp_conv_stream_launch(A, B, nullptr, nullptr, 0, batch, M, K, N, g.x_bs, g.w_bs, g.out_bs, C, N, stream);
    const bool narrow = pl.narrow, bk16 = pl.slab == 16;
    g.tiles_m = pl.tiles_m;
    g.tiles_n = pl.tiles_n;
    const int T = g.tiles_m * g.tiles_n;
    dim3 grid(8 * ((T + 7) / 8), batch);
#define CG_GOG(NT_, BK_, GL_) hipLaunchKernelGGL((conv_igemm_f32_kernel<NT_, 0, false, BK_, false, GL_>), grid, dim3(CG_THREADS), 0, emp_stream(stream), g)
    if (narrow) {
        if (pl.glds) { if (bk16) CG_GOG(1, 16, true); else CG_GOG(1, 32, true); }
        else { if (bk16) CG_GOG(1, 16, false); else CG_GOG(1, 32, false); }
    } else {
        if (pl.glds) { if (bk16) CG_GOG(2, 16, true); else CG_GOG(2, 32, true); }
        else { if (bk16) CG_GOG(2, 16, false); else CG_GOG(2, 32, false); }
    }
#undef CG_GOG
    EMP_CHECK_LAUNCH("emp_gemm_nt_batched");
    return EMP_OK;
}

extern "C" int emp_wino_gemm_fused(const float *x, int N, int H, int W, int Cin, int dil, const int32_t *tiles,
                                   int64_t T, const float *U, int Cout, float *Mw, void *stream)
{
    EMP_REQUIRE(x && tiles && U && Mw, "wino_gemm: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cin % CG_BK == 0 && Cout > 0 && dil >= 1 && T >= 0,
                "wino_gemm: bad shape (Cin must be a multiple of %d)", CG_BK);
    EMP_REQUIRE((int64_t)N * H * W * Cin < (1LL << 31) && T < (1LL << 31), "wino_gemm: activation too large for 32-bit offsets");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(U)) & 15) == 0, "wino_gemm: alignment");
    if (T == 0) return EMP_OK;
    ConvGeom g;
    g.x = x; g.w = U; g.scale = g.shift = g.res = nullptr; g.out = Mw;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.OH = 1; g.OW = 1; g.Cout = Cout; g.KH = g.KW = 1;
    g.stride = 1; g.pad = 0; g.dil = dil; g.relu = 0;
    g.M = T; g.out_ps = Cout; g.res_ps = Cout;
    g.x_bs = 0; g.w_bs = (int64_t)Cout * Cin; g.out_bs = T * Cout; g.tiles = tiles; g.proj_w = nullptr; g.proj_out = nullptr; g.proj_n = 0; g.hw = 1;
    const bool narrow = Cout <= 64;
    g.tiles_m = (int)emp_cdiv(T, CG_BM);
    g.tiles_n = (int)emp_cdiv(Cout, narrow ? 64 : 128);
    const int nt = g.tiles_m * g.tiles_n;
    dim3 grid(8 * ((nt + 7) / 8), 16);
    if (narrow) hipLaunchKernelGGL((conv_igemm_f32_kernel<1, 1>), grid, dim3(CG_THREADS), 0, emp_stream(stream), g);
    else hipLaunchKernelGGL((conv_igemm_f32_kernel<2, 1>), grid, dim3(CG_THREADS), 0, emp_stream(stream), g);
    EMP_CHECK_LAUNCH("emp_wino_gemm_fused");
    return EMP_OK;
}

extern "C" int emp_wino_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                                         int Cout, int dil, const float *scale, const float *shift, int relu,
                                         float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(Mw && tiles && out, "wino_output: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0 && dil >= 1 && T >= 0, "wino_output: bad shape");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout && out_pixel_stride % 4 == 0, "wino_output: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(Mw) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(scale) |
                  reinterpret_cast<uintptr_t>(shift)) & 15) == 0, "wino_output: alignment");
    if (T == 0) return EMP_OK;
    hipLaunchKernelGGL(wino_output_kernel, dim3(emp_grid(T * (Cout / 4), 256, 16384)), dim3(256), 0, emp_stream(stream),
                       reinterpret_cast<const float4 *>(Mw), tiles, T, H, W, Cout / 4, dil,
                       reinterpret_cast<const float4 *>(scale), reinterpret_cast<const float4 *>(shift), relu, out,
                       out_pixel_stride);
    EMP_CHECK_LAUNCH("emp_wino_output_transform");
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------
// D5b: Winograd F(4x4, 3x3): 36 position GEMMs, 4x fewer matrix-core FLOPs than the direct form (F(2x2,3x3):
// 2.25x).  Same decomposition as D5 (dilation = sub-grids, tile table from the host: patch origin (n, y, x), a tile
// now covers 4x4 outputs of its sub-grid and reads a 6x6 patch).  The transforms amplify rounding by about 10x
// relative to the direct form (measured 1.3e-6 * sum|x||w| at K = 18432), so this variant is tested against a
// looser stated tolerance and offered to the tuner only as an alternative.
// The transforms themselves (B^T, A^T, one fp32 rounding per operation, columns first, then rows) and the v4 helpers
// are in emp_wino4.h, shared with the one-kernel path (emp_wino4.hip, D5d).

// x (N,H,W,C) -> V (36, T, C); one thread per (tile, 4 channels)
__global__ __launch_bounds__(256) void wino4_input_kernel(const float *__restrict__ x, const int32_t *__restrict__ tiles,
                                                          int64_t T, int H, int W, int C4, int dil, float4 *__restrict__ V)
{
    const int64_t total = T * C4;
    // XCD-aware block order (the grid is a multiple of 8): consecutive hardware block ids go to different XCDs, each with
    // its own L2, while consecutive TILE ROWS share two of their six patch rows.  Logical block lb = the (b >> 3)-th of
    // XCD (b & 7)'s contiguous range, so that the rows a patch shares with the tile row above are still in the L2 of
    // the XCD that fetched them (round 2 measured the input being read 1.6x: neighbouring tile rows sat on different XCDs).
    const int64_t chunk = gridDim.x >> 3;
    const int64_t lb = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    for (int64_t i = lb * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const int64_t t = i / C4;
        const int n = tiles[3 * t], by = tiles[3 * t + 1], bx = tiles[3 * t + 2];
        const float4 *src = reinterpret_cast<const float4 *>(x) + (int64_t)n * H * W * C4 + c4;
        v4 tt[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {          // along columns: t[a] = d[a] B
            v4 d[6];
            const int yy = by + a * dil;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int xx = bx + b * dil;
                d[b] = {0.f, 0.f, 0.f, 0.f};
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) d[b] = ldv4(src + ((int64_t)yy * W + xx) * C4);
            }
            wino4_bt(d, tt[a]);
        }
        float4 *dst = V + t * C4 + c4;
        const int64_t ps = T * C4;             // position stride
#pragma unroll
        for (int v = 0; v < 6; ++v) {          // along rows: V = B^T t
            v4 col[6], r[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) col[a] = tt[a][v];
            wino4_bt(col, r);
#pragma unroll
            for (int u = 0; u < 6; ++u) stv4(dst + (u * 6 + v) * ps, r[u]);
        }
    }
}

// Mw (36, T, Cout) -> out (N,H,W,Cout) with the fused epilogue; one thread per (tile, 4 couts)
__global__ __launch_bounds__(256) void wino4_output_kernel(const float4 *__restrict__ Mw, const int32_t *__restrict__ tiles,
                                                           int64_t T, int H, int W, int Co4, int dil,
                                                           const float4 *__restrict__ scale, const float4 *__restrict__ shift,
                                                           int relu, float *__restrict__ out, int64_t out_ps)
{
    const int64_t total = T * Co4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % Co4);
        const int64_t t = i / Co4;
        const int n = tiles[3 * t], oy = tiles[3 * t + 1] + dil, ox = tiles[3 * t + 2] + dil;
        const float4 *src = Mw + t * Co4 + c4;
        const int64_t ps = T * Co4;
        v4 s[4][6];
#pragma unroll
        for (int b = 0; b < 6; ++b) {          // rows: s = A^T m
            v4 m[6], r[4];
#pragma unroll
            for (int a = 0; a < 6; ++a) m[a] = ldv4(src + (a * 6 + b) * ps);
            wino4_at(m, r);
#pragma unroll
            for (int a = 0; a < 4; ++a) s[a][b] = r[a];
        }
        v4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (scale) sc = ldv4(scale + c4);
        if (shift) sh = ldv4(shift + c4);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            v4 yv[4];
            wino4_at(s[a], yv);                // columns: y = s A
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int yy = oy + a * dil, xx = ox + b * dil;
                if (yy < H && xx < W) {
                    v4 v = yv[b];
                    if (scale) v = {__fmul_rn(v.x, sc.x), __fmul_rn(v.y, sc.y), __fmul_rn(v.z, sc.z), __fmul_rn(v.w, sc.w)};
                    if (shift) v = v + sh;
                    if (relu) v = {fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
                    stv4(reinterpret_cast<float4 *>(out + (((int64_t)n * H + yy) * W + xx) * out_ps + 4 * c4), v);
                }
            }
        }
    }
}

extern "C" int emp_wino4_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                                         int64_t T, float *V, void *stream)
{
    EMP_REQUIRE(x && tiles && V, "wino4_input: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && dil >= 1 && T >= 0, "wino4_input: bad shape");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(V)) & 15) == 0, "wino4_input: alignment");
    if (T == 0) return EMP_OK;
    const int grid = (emp_grid(T * (C / 4), 256, 16384) + 7) / 8 * 8;           // a multiple of 8: see the block order
    hipLaunchKernelGGL(wino4_input_kernel, dim3(grid), dim3(256), 0, emp_stream(stream), x, tiles, T, H, W, C / 4, dil,
                       reinterpret_cast<float4 *>(V));
    EMP_CHECK_LAUNCH("emp_wino4_input_transform");
    return EMP_OK;
}

extern "C" int emp_wino4_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                                          int Cout, int dil, const float *scale, const float *shift, int relu,
                                          float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(Mw && tiles && out, "wino4_output: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0 && dil >= 1 && T >= 0, "wino4_output: bad shape");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout && out_pixel_stride % 4 == 0, "wino4_output: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(Mw) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(scale) |
                  reinterpret_cast<uintptr_t>(shift)) & 15) == 0, "wino4_output: alignment");
    if (T == 0) return EMP_OK;
    hipLaunchKernelGGL(wino4_output_kernel, dim3(emp_grid(T * (Cout / 4), 256, 16384)), dim3(256), 0, emp_stream(stream),
                       reinterpret_cast<const float4 *>(Mw), tiles, T, H, W, Cout / 4, dil,
                       reinterpret_cast<const float4 *>(scale), reinterpret_cast<const float4 *>(shift), relu, out,
                       out_pixel_stride);
    EMP_CHECK_LAUNCH("emp_wino4_output_transform");
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------
// D5c: Winograd F(3x3, 3x3) (points 0, 1, -1, 2, inf): 5x5 patches, 25 position GEMMs, 3x3 outputs per tile, 3.24x
// fewer matrix-core FLOPs than the direct form.  It exists for the dilation-6 ASPP branch on 32-pixel maps: the
// sub-grids have 5 or 6 rows, which two 3-row tiles cover almost exactly, while 4-row tiles waste half and 2-row
// tiles need 3.  Transforms written generically: r[u] = left fold over the non-zero entries of row u (ascending
// index) of c * d, every product and every sum one fp32 rounding.
//   B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]      A^T = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 1]
//   G   = [1/2 0 0; -1/2 -1/2 -1/2; -1/6 1/6 -1/6; 1/6 1/3 2/3; 0 0 1]  (host, fp64, rounded once)
__device__ __forceinline__ void wino3_fold(const float (&c)[5], const v4 d[5], v4 &out)
{
    bool first = true;
    out = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        if (c[a] != 0.f) {
            const v4 term = c[a] * d[a];
            out = first ? term : out + term;
            first = false;
        }
    }
}

__device__ __forceinline__ void wino3_bt(const v4 d[5], v4 r[5])
{
    constexpr float BT[5][5] = {{2, -1, -2, 1, 0}, {0, -2, -1, 1, 0}, {0, 2, -3, 1, 0}, {0, -1, 0, 1, 0}, {0, 2, -1, -2, 1}};
#pragma unroll
    for (int u = 0; u < 5; ++u) wino3_fold(BT[u], d, r[u]);
}

__device__ __forceinline__ void wino3_at(const v4 m[5], v4 s[3])
{
    constexpr float AT[3][5] = {{1, 1, 1, 1, 0}, {0, 1, -1, 2, 0}, {0, 1, 1, 4, 1}};
#pragma unroll
    for (int u = 0; u < 3; ++u) wino3_fold(AT[u], m, s[u]);
}

__global__ __launch_bounds__(256) void wino3_input_kernel(const float *__restrict__ x, const int32_t *__restrict__ tiles,
                                                          int64_t T, int H, int W, int C4, int dil, float4 *__restrict__ V)
{
    const int64_t total = T * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const int64_t t = i / C4;
        const int n = tiles[3 * t], by = tiles[3 * t + 1], bx = tiles[3 * t + 2];
        const float4 *src = reinterpret_cast<const float4 *>(x) + (int64_t)n * H * W * C4 + c4;
        v4 tt[5][5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            v4 d[5];
            const int yy = by + a * dil;
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                const int xx = bx + b * dil;
                d[b] = {0.f, 0.f, 0.f, 0.f};
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) d[b] = ldv4(src + ((int64_t)yy * W + xx) * C4);
            }
            wino3_bt(d, tt[a]);
        }
        float4 *dst = V + t * C4 + c4;
        const int64_t ps = T * C4;
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            v4 col[5], r[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) col[a] = tt[a][v];
            wino3_bt(col, r);
#pragma unroll
            for (int u = 0; u < 5; ++u) stv4(dst + (u * 5 + v) * ps, r[u]);
        }
    }
}

__global__ __launch_bounds__(256) void wino3_output_kernel(const float4 *__restrict__ Mw, const int32_t *__restrict__ tiles,
                                                           int64_t T, int H, int W, int Co4, int dil,
                                                           const float4 *__restrict__ scale, const float4 *__restrict__ shift,
                                                           int relu, float *__restrict__ out, int64_t out_ps)
{
    const int64_t total = T * Co4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % Co4);
        const int64_t t = i / Co4;
        const int n = tiles[3 * t], oy = tiles[3 * t + 1] + dil, ox = tiles[3 * t + 2] + dil;
        const float4 *src = Mw + t * Co4 + c4;
        const int64_t ps = T * Co4;
        v4 s[3][5];
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            v4 m[5], r[3];
#pragma unroll
            for (int a = 0; a < 5; ++a) m[a] = ldv4(src + (a * 5 + b) * ps);
            wino3_at(m, r);
#pragma unroll
            for (int a = 0; a < 3; ++a) s[a][b] = r[a];
        }
        v4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (scale) sc = ldv4(scale + c4);
        if (shift) sh = ldv4(shift + c4);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v4 yv[3];
            wino3_at(s[a], yv);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int yy = oy + a * dil, xx = ox + b * dil;
                if (yy < H && xx < W) {
                    v4 v = yv[b];
                    if (scale) v = {__fmul_rn(v.x, sc.x), __fmul_rn(v.y, sc.y), __fmul_rn(v.z, sc.z), __fmul_rn(v.w, sc.w)};
                    if (shift) v = v + sh;
                    if (relu) v = {fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
                    stv4(reinterpret_cast<float4 *>(out + (((int64_t)n * H + yy) * W + xx) * out_ps + 4 * c4), v);
                }
            }
        }
    }
}

extern "C" int emp_wino3_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                                         int64_t T, float *V, void *stream)
{
    EMP_REQUIRE(x && tiles && V, "wino3_input: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && dil >= 1 && T >= 0, "wino3_input: bad shape");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(V)) & 15) == 0, "wino3_input: alignment");
    if (T == 0) return EMP_OK;
    hipLaunchKernelGGL(wino3_input_kernel, dim3(emp_grid(T * (C / 4), 256, 16384)), dim3(256), 0, emp_stream(stream), x,
                       tiles, T, H, W, C / 4, dil, reinterpret_cast<float4 *>(V));
    EMP_CHECK_LAUNCH("emp_wino3_input_transform");
    return EMP_OK;
}

extern "C" int emp_wino3_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                                          int Cout, int dil, const float *scale, const float *shift, int relu,
                                          float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(Mw && tiles && out, "wino3_output: null pointer");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0 && dil >= 1 && T >= 0, "wino3_output: bad shape");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout && out_pixel_stride % 4 == 0, "wino3_output: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(Mw) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(scale) |
                  reinterpret_cast<uintptr_t>(shift)) & 15) == 0, "wino3_output: alignment");
    if (T == 0) return EMP_OK;
    hipLaunchKernelGGL(wino3_output_kernel, dim3(emp_grid(T * (Cout / 4), 256, 16384)), dim3(256), 0, emp_stream(stream),
                       reinterpret_cast<const float4 *>(Mw), tiles, T, H, W, Cout / 4, dil,
                       reinterpret_cast<const float4 *>(scale), reinterpret_cast<const float4 *>(shift), relu, out,
                       out_pixel_stride);
    EMP_CHECK_LAUNCH("emp_wino3_output_transform");
    return EMP_OK;
}
