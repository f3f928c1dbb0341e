// D4c: persistent tile-stream form of the tiled fp32 implicit-GEMM kernel (emp_conv.hip) for its GEMM-shaped launches:
// 1x1, stride 1, no padding, K-slab 16, LDS-direct staging, 128 x 128 tiles, no residual.  gfx950 only.
//
//   The one-tile-per-block kernel pays a fixed cost per output tile that does not depend on K (a fresh block's address
//   set-up and first-slab latency, the fill and drain of the slab ring, an epilogue through LDS with three to five block
//   barriers): 1/TF = a + b/K over its launches.  Here a block lives for the whole launch and walks a sequence of tiles:
//     * grid = the resident blocks (three per CU: 768), block b stays on XCD b & 7 and walks the tiles of that XCD's
//       contiguous chunk, b >> 3, b >> 3 + grid / 8, ... (cs_walk): the numbering of emp_conv.hip, so the cout tiles
//       of one pixel tile are still fetched by neighbours in time on one XCD.  A batch (emp_gemm_nt_batched) is folded
//       into the sequence: unit u = entry * tiles + tile;
//     * ONE slab stream: the ring of three LDS slabs and the two-slabs-ahead LDS-direct loads run on over tile
//       boundaries -- the loads of the next tile's first two slabs are issued during this tile's last two iterations;
//       tiles shorter than the ring (K = 16, 32) simply put more than one boundary inside the prefetch distance;
//     * the epilogue does not touch LDS: in the 32x32 C/D map a lane is a cout and a register a pixel row, so each
//       global_store_dword writes two 128-byte row segments straight from the accumulators; no barrier belongs to it.
//   Inside a tile the slab order and the k-step order (channels j and 8 + j) are those of conv_igemm_f32_kernel<2, 0,
//   false, 16, false, true>, the epilogue is the same __fmul_rn / __fadd_rn / fmaxf: results are bit-identical and
//   emp_conv_k_slab* keep their answers.
#include "emp_common.h"
#include <atomic>
#include <stdlib.h>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CS_BM 128
#define CS_BN 128
#define CS_BK 16
#define CS_THREADS 256
#define CS_RING 3
#define CS_RESIDENT 768       // 256 CUs x 3 blocks (49 152 B of LDS and <= 168 registers each)

struct StreamGeom {
    const float *x, *w, *scale, *shift;
    float *out;
    int Cin, Cout, tiles_n;
    int64_t M, out_ps;
    int64_t tiles, total;            // tiles per batch entry (pixel tiles x cout tiles), entries x tiles
    int64_t x_bs, w_bs, out_bs;      // element strides of a batch entry
};

// The walk: unit (entry * tiles + tile) that block b of a grid of `grid` blocks (a multiple of 8) works on in its step
// `step`, or -1 when the block has no such step.  XCD b & 7 owns the units [x * chunk, (x + 1) * chunk).
__host__ __device__ static inline int64_t cs_walk(int64_t total, int grid, int b, int64_t step)
{
    const int64_t chunk = (total + 7) >> 3;
    const int64_t local = (b >> 3) + step * (grid >> 3);
    if (local >= chunk) return -1;
    const int64_t u = (b & 7) * chunk + local;
    return u < total ? u : -1;
}
// steps block b has (its units ascend with the step, so the valid steps are a prefix)
__host__ __device__ static inline int64_t cs_walk_steps(int64_t total, int grid, int b)
{
    const int64_t chunk = (total + 7) >> 3;
    int64_t end = total - (b & 7) * chunk;            // units of this XCD's chunk that exist
    if (end > chunk) end = chunk;
    const int64_t first = b >> 3, stride = grid >> 3;
    return end > first ? (end - first + stride - 1) / stride : 0;
}

extern "C" int emp_conv_stream_walk(int64_t tiles, int batch, int grid, int block, int64_t step, int64_t *entry, int64_t *tile)
{
    if (tiles <= 0 || batch <= 0 || grid <= 0 || (grid & 7) || block < 0 || block >= grid || step < 0) return 0;
    const int64_t u = cs_walk(tiles * batch, grid, block, step);
    if (u < 0 || step >= cs_walk_steps(tiles * batch, grid, block)) return 0;
    if (entry) *entry = u / tiles;
    if (tile) *tile = u % tiles;
    return 1;
}

// the grid a launch of `total` units gets: the resident blocks, or fewer when there are fewer units
static inline int cs_grid(int64_t total)
{
    const int64_t g = 8 * ((total + 7) / 8);
    return (int)(g < CS_RESIDENT ? g : CS_RESIDENT);
}
extern "C" int emp_conv_stream_grid(int64_t tiles, int batch) { return tiles > 0 && batch > 0 ? cs_grid(tiles * batch) : 0; }

// 16 bytes per lane from global memory (block-uniform base + the lane's byte offset) straight into LDS: lane l's data
// lands at lds_byte_addr + 16 * l.  Not tracked by the compiler: pair with cs_wait_vm.
__device__ __forceinline__ void cs_glds16(const float *base, unsigned lane_off, unsigned lds_byte_addr)
{
    // s_nop 4: the base may have been written by a VALU instruction (v_readlane of a spilled SGPR) right before
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(base), "s"(lds_byte_addr) : "memory", "m0");
}
// the epilogue's stores of one accumulator row: couts r and 32 + r of the wave's 64, one address
__device__ __forceinline__ void cs_store2(float *dst, float v0, float v1)
{
    asm volatile("global_store_dword %0, %1, off\n\tglobal_store_dword %0, %2, off offset:128" ::"v"(dst), "v"(v0), "v"(v1) : "memory");
}
template <int N>
__device__ __forceinline__ void cs_wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// AFFINE: out = relu?(acc * scale + shift) (both required); else out = acc (the batched GEMM)
template <bool AFFINE, bool RELU>
__global__ __launch_bounds__(CS_THREADS, 3) void conv_stream_f32_kernel(StreamGeom g)
{
    constexpr int BK = CS_BK, TPR = BK / 4, RPP = CS_THREADS / TPR, AR = CS_BM / RPP, BROWS = CS_BN / RPP;
    constexpr int NF4 = BK / 8, RPW = 64 / TPR, NL = AR + BROWS;                  // LDS-direct loads per slab and lane
    constexpr int A_ELEMS = CS_RING * CS_BM * BK, B_ELEMS = CS_RING * CS_BN * BK;
    __shared__ __attribute__((aligned(16))) float smem[A_ELEMS + B_ELEMS];
    float *As = smem, *Bs = smem + A_ELEMS;

    // everything that shapes the control flow below (nt, S, n_slabs, the cursors) derives from blockIdx and the kernel
    // arguments alone: the trip count and every barrier are block-uniform by construction
    const int b = blockIdx.x, grid = gridDim.x;
    const int nt = (int)cs_walk_steps(g.total, grid, b);
    if (nt == 0) return;
    const int S = g.Cin / BK;
    const int n_slabs = nt * S;                          // the launcher keeps this below 2^31
    const int64_t u0 = cs_walk(g.total, grid, b, 0);
    const int64_t ustep = grid >> 3;

    const int tid = threadIdx.x;
    const int lrow = tid / TPR;
    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, hh = lane >> 5;
    const int csw = (((tid % TPR) ^ ((lrow >> 2) & 3)) * 4);      // logical chunk this lane fetches (floats)
    const int swz_rd = (r >> 2) & 3;

    // tile of a unit: entry, first pixel row, first cout
    auto locate = [&](int64_t u, int64_t &entry, int64_t &m0, int &n0) {
        // total < 2^28 (launcher): 32-bit divisions, and none for the entry without a batch
        const unsigned uu = (unsigned)u, tiles = (unsigned)g.tiles, tn_ = (unsigned)g.tiles_n;
        const unsigned e = g.total == g.tiles ? 0u : uu / tiles;
        const unsigned t = uu - e * tiles;
        const unsigned tm = t / tn_;
        entry = e;
        m0 = (int64_t)tm * CS_BM;
        n0 = (int)(t - tm * tn_) * CS_BN;
    };

    // ---- load cursor: the next slab to request ------------------------------------------------------------------
    // A block-uniform base per operand (SGPRs, advanced slab by slab) plus a 32-bit lane offset.  Rows past M are clamped
    // to the last row: they multiply into accumulator rows that are never stored, and no lane reads outside x.
    const float *a_base = nullptr, *b_base = nullptr;
    unsigned voff_a[AR];
    const unsigned voff_b = (unsigned)(lrow * g.Cin + csw) * 4u;
    int ld_k = 0, ld_c0 = 0, ld_ring = 0;
    auto set_ld_tile = [&](int k) {
        int64_t entry, m0;
        int n0;
        locate(u0 + k * ustep, entry, m0, n0);
        a_base = g.x + entry * g.x_bs + m0 * g.Cin;
        b_base = g.w + entry * g.w_bs + (int64_t)n0 * g.Cin;       // Cout is a multiple of 128: every row of a cout tile exists
        const int last = (int)(g.M - m0 < CS_BM ? g.M - m0 : CS_BM) - 1;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int row = lrow + RPP * i;
            voff_a[i] = (unsigned)((row < last ? row : last) * g.Cin + csw) * 4u;
        }
    };
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)smem;
    const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(RPW * wave * BK * 4));
    const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((A_ELEMS + RPW * wave * BK) * 4));
    auto issue_slab = [&]() {
#pragma unroll
        for (int i = 0; i < AR; ++i)
            cs_glds16(a_base + ld_c0, voff_a[i], a_dst + (unsigned)((ld_ring * CS_BM + RPP * i) * BK * 4));
#pragma unroll
        for (int i = 0; i < BROWS; ++i)
            cs_glds16(b_base + (int64_t)(RPP * i) * g.Cin + ld_c0, voff_b, b_dst + (unsigned)((ld_ring * CS_BN + RPP * i) * BK * 4));
        ld_ring = ld_ring == CS_RING - 1 ? 0 : ld_ring + 1;
        ld_c0 += BK;
        if (ld_c0 == g.Cin) {                  // block-uniform: on to the next tile of the walk
            ld_c0 = 0;
            ++ld_k;
            if (ld_k < nt) set_ld_tile(ld_k);
        }
    };

    // ---- compute cursor ----------------------------------------------------------------------------------------
    int cp_k = 0, cp_s = 0, rd_ring = 0;
    int sc_n0 = -1;                            // cout tile whose scale / shift the lane holds
    float sc[2] = {1.f, 1.f}, sh[2] = {0.f, 0.f};
    // Ordinary (compiler-tracked) loads; the compiler waits vmcnt(0) at their use, which also drains every LDS-direct
    // load in flight.  The use is forced HERE (the empty asm), so the drain happens where this is called and nowhere
    // later: before the first slab is requested, and again only when a block's walk changes cout tile -- never when
    // grid / 8 = 96 is a multiple of the cout tiles (Cout 128, 256, 384, 512, 1024, 2048: all the models' sites).
    auto load_affine = [&](int n0) {
        if constexpr (AFFINE) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                sc[j] = g.scale[n0 + wn * 64 + j * 32 + r];
                sh[j] = g.shift[n0 + wn * 64 + j * 32 + r];
            }
            asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(sh[0]), "+v"(sh[1]));
        }
        sc_n0 = n0;
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    // y = relu?(acc * scale + shift), row (pixel) = 32 i + (q & 3) + 8 (q >> 2) + 4 hh of the wave's 64, col (cout) =
    // 32 j + r of its 64.
    auto epilogue = [&](int k) {
        int64_t entry, m0;
        int n0;
        locate(u0 + k * ustep, entry, m0, n0);
        if (n0 != sc_n0) load_affine(n0);      // block-uniform
        float *obase = g.out + entry * g.out_bs + (m0 + wm * 64 + 4 * hh) * g.out_ps + n0 + wn * 64 + r;
        const bool whole = m0 + CS_BM <= g.M;  // block-uniform
        auto rows = [&](auto checked) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = i * 32 + (q & 3) + 8 * (q >> 2);
                    float v[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        v[j] = acc[i][j][q];
                        if constexpr (AFFINE) v[j] = __fadd_rn(__fmul_rn(v[j], sc[j]), sh[j]);
                        if constexpr (RELU) v[j] = fmaxf(v[j], 0.f);
                    }
                    if (!decltype(checked)::value || m0 + wm * 64 + 4 * hh + row < g.M) cs_store2(obase + row * g.out_ps, v[0], v[1]);
                }
        };
        if (whole) rows(std::false_type{}); else rows(std::true_type{});
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    };

    {
        int64_t entry, m0;
        int n0;
        locate(u0, entry, m0, n0);
        load_affine(n0);
    }
    set_ld_tile(0);

    // Vector-memory operations of a wave, in issue order; LDS-direct loads and stores both sit on the one counter:
    //   [the scale / shift loads: retired before the first LDS-direct load is issued, see load_affine]
    //   L(0), L(1)                                   prologue; L(s) = the NL LDS-direct loads of stream slab s
    //   iteration s:  L(s + 2) at its top (if the stream has such a slab), then the MFMAs of slab s, then WAIT, barrier,
    //                 and -- when slab s is its tile's last -- E(s): up to 64 stores per lane
    //   WAIT of iteration s must retire L(s + 1), issued at the top of iteration s - 1.  Issued after it: E(s - 1), if
    //   slab s - 1 ended a tile, and L(s + 2), if it exists.  The wait is vmcnt(NL) if L(s + 2) exists, else vmcnt(0):
    //     * loads retire in order among themselves, so "at most NL operations pending" leaves no load of L(s + 1) pending
    //       -- whether or not stores retire in order with loads, which this loop therefore does not rely on;
    //     * it also asks for every store of E(s - 1) to be complete.  They were issued before the MFMAs of slab s (at
    //       least 2 048 cycles of this wave's matrix time, three times that with three resident blocks), and a tile ends
    //       once per Cin / 16 iterations; counting them instead (vmcnt(63) would let all but 1 or 5 of them stay
    //       pending IF the counter is in order across loads and stores) is not worth resting on that.
    //   A reload of scale / shift inside E (cout tile changed) drains everything; the waits then only ask for less than
    //   has already happened.  With K = 16 or 32 several tiles end inside the prefetch distance; the rule above is per
    //   iteration and does not care.
    issue_slab();
    if (n_slabs > 1) issue_slab();
    if (n_slabs > 1) cs_wait_vm<NL>(); else cs_wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    for (int s = 0; s < n_slabs; ++s) {
        const bool more = s + 2 < n_slabs;
        if (more) issue_slab();                // into the slot read in iteration s - 1 (barrier at its end)
        const float *Ar = &As[rd_ring * CS_BM * BK + (wm * 64 + r) * BK];
        const float *Br = &Bs[rd_ring * CS_BN * BK + (wn * 64 + r) * BK];
#pragma unroll
        for (int f = 0; f < NF4; ++f) {
            const int pc = (((hh * NF4 + f) ^ swz_rd) * 4);         // physical position of logical chunk hh*NF4 + f
            float4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4 *>(Ar + i * 32 * BK + pc);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const float4 *>(Br + j * 32 * BK + pc);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float av[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) av[i] = e == 0 ? fa[i].x : e == 1 ? fa[i].y : e == 2 ? fa[i].z : fa[i].w;
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = e == 0 ? fb[j].x : e == 1 ? fb[j].y : e == 2 ? fb[j].z : fb[j].w;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
        rd_ring = rd_ring == CS_RING - 1 ? 0 : rd_ring + 1;
        if (more) cs_wait_vm<NL>(); else cs_wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        if (++cp_s == S) {                     // block-uniform
            epilogue(cp_k);
            cp_s = 0;
            ++cp_k;
        }
    }
}

static std::atomic<int64_t> cs_launches;
extern "C" int64_t emp_conv_stream_launches(void) { return cs_launches.load(); }

// called by the launchers of emp_conv.hip for launches emp_conv_stream_eligible admits (operands checked there)
extern "C" __attribute__((visibility("hidden"))) int emp_conv_stream_launch(const float *x, const float *w, const float *scale, const float *shift,
                                                                            int relu, int batch, int64_t M, int Cin, int Cout,
                                                                            int64_t x_bs, int64_t w_bs, int64_t out_bs, float *out,
                                                                            int64_t out_ps, void *stream)
{
    EMP_REQUIRE(x && w && out && (scale != nullptr) == (shift != nullptr), "conv_stream: null pointer");
    EMP_REQUIRE(batch >= 1 && M > 0 && Cin > 0 && Cin % CS_BK == 0 && Cout > 0 && Cout % CS_BN == 0, "conv_stream: bad shape");
    EMP_REQUIRE(scale || !relu, "conv_stream: ReLU needs scale and shift");
    StreamGeom g;
    g.x = x; g.w = w; g.scale = scale; g.shift = shift; g.out = out;
    g.Cin = Cin; g.Cout = Cout; g.tiles_n = Cout / CS_BN;
    g.M = M; g.out_ps = out_ps;
    g.tiles = emp_cdiv(M, CS_BM) * g.tiles_n;
    g.total = g.tiles * batch;
    g.x_bs = x_bs; g.w_bs = w_bs; g.out_bs = out_bs;
    const int grid = cs_grid(g.total);
    EMP_REQUIRE(g.total < (1LL << 28) && (g.total / grid + 2) * (Cin / CS_BK) < (1LL << 30), "conv_stream: too many tiles");
    hipStream_t st = emp_stream(stream);
    if (!scale) hipLaunchKernelGGL((conv_stream_f32_kernel<false, false>), dim3(grid), dim3(CS_THREADS), 0, st, g);
    else if (relu) hipLaunchKernelGGL((conv_stream_f32_kernel<true, true>), dim3(grid), dim3(CS_THREADS), 0, st, g);
    else hipLaunchKernelGGL((conv_stream_f32_kernel<true, false>), dim3(grid), dim3(CS_THREADS), 0, st, g);
    EMP_CHECK_LAUNCH("emp_conv_stream_launch");
    ++cs_launches;
    return EMP_OK;
}
