// Zlib streams of label slices, made on the device: one zarr chunk (one slice of uint8 or uint32 labels) becomes one
// stream any inflate reads.  replaces zarr's default compressor behind zarr_store.create_dataset
// (scripts/pdl_inference3d.py:228-233), which the reference runs on the CPU; the format is in include/emp_hip.h.
//
// Same shape as the run extractor of emp_runs.hip: count (exact compressed bytes and Adler-32 partial sums per
// segment), scan (byte offset of every segment), write (the same tokens again, now with their bit positions).  A
// segment is DF_SEG raw bytes and one wave; it ends byte-aligned, so segments and chunks are concatenated as bytes.
// The coder needs no hash table and no history search: an element equal to the one before it is part of a repeat, and
// a repeat is a match at distance `item`; everything else is literal bytes under the fixed Huffman code.
// Per raw byte each pass reads one byte; the encode pass writes the compressed bytes once.  All else is per segment.
#include "emp_common.h"

#define DF_SEG 4096                              // raw bytes per segment (a multiple of 16: DF_ROUNDS rounds of 1 KiB)
#define DF_ROUNDS (DF_SEG / 1024)                // a round = 64 lanes x 16 bytes
#define DF_MASK_WORDS (DF_SEG / 32 + 4)          // one "repeats its predecessor" bit per element + a zero word that ends every search
#define DF_SEG_MAX_BYTES (2 + (13 + 9 * DF_SEG + 7) / 8 + 4 + 6)   // header, all-literal block, stored block, trailer
#define DF_BUF_LINES ((DF_SEG_MAX_BYTES + 15 + 15) / 16 + 2)       // 16-byte lines of the bit buffer (15: the output's misalignment)
#define DF_MOD 65521u

static_assert(DF_SEG % 1024 == 0, "a segment is a whole number of rounds");

static int64_t df_bound(int64_t L) { return 2 + (9 * L + 7) / 8 + 8 * emp_cdiv(L, DF_SEG) + 6; }

// ------------------------------------------------------------------------------------------ the fixed Huffman code
// All values are in STREAM order: deflate fills bytes from the least significant bit, Huffman codes go in most
// significant bit first (hence __brev), extra bits least significant first (RFC 1951 3.1.1, 3.2.5, 3.2.6).
__device__ __forceinline__ uint32_t df_lit_bits(uint32_t b) { return 8u + (b >= 144u ? 1u : 0u); }
__device__ __forceinline__ uint32_t df_lit_code(uint32_t b)
{
    return b < 144u ? (__brev(0x30u + b) >> 24) : (__brev(0x190u + (b - 144u)) >> 23);
}

// one match of len (3..258) bytes: length symbol, its extra bits, the 5-bit distance code (dist_rev, no extra bits)
__device__ __forceinline__ uint32_t df_match(uint32_t len, uint32_t dist_rev, uint32_t &nbits)
{
    const uint32_t l = len - 3u;
    uint32_t eb = 0u, sym;
    if (len == 258u) sym = 285u;
    else if (l < 8u) sym = 257u + l;
    else {
        eb = 29u - (uint32_t)__clz((int)l);      // floor(log2 l) - 2
        sym = 261u + 4u * eb + ((l >> eb) & 3u);
    }
    const uint32_t cb = sym < 280u ? 7u : 8u;
    const uint32_t code = sym < 280u ? (__brev(sym - 256u) >> 25) : (__brev(0xC0u + (sym - 280u)) >> 24);
    nbits = cb + eb + 5u;
    return code | ((l & ((1u << eb) - 1u)) << cb) | (dist_rev << (cb + eb));
}

// bits into the zeroed buffer; OR is order-free, so the bytes do not depend on which lane comes first
__device__ __forceinline__ void df_put(uint32_t *buf, uint32_t pos, uint32_t v, uint32_t nbits)
{
    const uint32_t wd = pos >> 5, s = pos & 31u;
    atomicOr(&buf[wd], v << s);
    if (s + nbits > 32u) atomicOr(&buf[wd + 1], v >> (32u - s));
}
__device__ __forceinline__ void df_put_byte(uint32_t *buf, uint32_t byte_pos, uint32_t v)
{
    atomicOr(&buf[byte_pos >> 2], v << (8u * (byte_pos & 3u)));
}

// A maximal repeat of n >= 3 bytes: 258s while n >= 261 or n == 258, then 259 / 260 as (n - 3, 3), then one match.
// Returns its bits; EMIT writes them at pos.
template <bool EMIT>
__device__ __forceinline__ uint32_t df_repeat(uint32_t n, uint32_t dist_rev, uint32_t *buf, uint32_t pos)
{
    const uint32_t k = n >= 261u ? (n - 3u) / 258u : 0u;
    const uint32_t r = n - 258u * k;              // 3..260
    uint32_t bits = 13u * k, nb;
    if (EMIT) {
        const uint32_t full = df_match(258u, dist_rev, nb);
        for (uint32_t i = 0; i < k; ++i) { df_put(buf, pos, full, 13u); pos += 13u; }
    }
    const uint32_t first = r > 258u ? r - 3u : r;
    uint32_t v = df_match(first, dist_rev, nb);
    if (EMIT) { df_put(buf, pos, v, nb); pos += nb; }
    bits += nb;
    if (r > 258u) {
        v = df_match(3u, dist_rev, nb);
        if (EMIT) df_put(buf, pos, v, nb);
        bits += nb;
    }
    return bits;
}

// The tokens that START in a lane's 16 bytes of a round (elements e0 .. e0 + nvalid of the segment): a literal element,
// or a repeat whose first element is here and whose end the flag mask gives.  One function for both passes: the count
// pass adds the bits up, the encode pass calls it a second time with EMIT and the position its prefix sum gave.
template <int ITEM, bool EMIT>
__device__ __forceinline__ uint32_t df_walk(const uint32_t (&w)[4], uint32_t e0, int nvalid, const uint32_t *mask,
                                            uint32_t *buf, uint32_t pos)
{
    constexpr int FL = 16 / ITEM;
    constexpr uint32_t DREV = ITEM == 1 ? 0u : 0x18u;        // distance code 0 (distance 1) / 3 (distance 4), reversed
    if (nvalid <= 0) return 0u;
    const uint32_t m = (mask[e0 >> 5] >> (e0 & 31u)) & ((1u << FL) - 1u);
    const uint32_t before = e0 ? (mask[(e0 - 1u) >> 5] >> ((e0 - 1u) & 31u)) & 1u : 0u;
    // a token starts at every valid element that is not the continuation of a repeat; in labels most lanes have none,
    // so only the set bits are visited
    uint32_t starts = ~(m & ((m << 1) | before)) & ((1u << nvalid) - 1u);
    uint32_t bits = 0u;
    while (starts) {
        const int j = __ffs((int)starts) - 1;
        starts &= starts - 1u;
        const uint32_t rep = (m >> j) & 1u;
        const int q = ITEM == 4 ? j : j >> 2;
        const uint32_t word = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
        const uint32_t v = ITEM == 4 ? word : (word >> (8 * (j & 3))) & 0xffu;
        uint32_t n = ITEM;                                   // bytes this token covers as literals, unless it is a repeat of >= 3
        if (rep) {
            const uint32_t p = e0 + j + 1u;                  // the first element after this one that does not repeat
            uint32_t wd = p >> 5;
            uint32_t x = ~mask[wd] & (0xffffffffu << (p & 31u));
            while (!x) x = ~mask[++wd];
            n = ((wd << 5) + (uint32_t)__ffs((int)x) - 1u - (e0 + j)) * ITEM;
        }
        uint32_t t;
        if (rep && n >= 3u) {
            t = df_repeat<EMIT>(n, DREV, buf, pos);
        } else if (ITEM == 4) {
            const uint32_t b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
            const uint32_t n0 = df_lit_bits(b0), n1 = df_lit_bits(b1), n2 = df_lit_bits(b2), n3 = df_lit_bits(b3);
            if (EMIT) {
                df_put(buf, pos, df_lit_code(b0) | (df_lit_code(b1) << n0), n0 + n1);
                df_put(buf, pos + n0 + n1, df_lit_code(b2) | (df_lit_code(b3) << n2), n2 + n3);
            }
            t = n0 + n1 + n2 + n3;
        } else {                                             // one byte, or a repeat of 1 or 2 bytes written out
            const uint32_t nb = df_lit_bits(v);
            if (EMIT) {
                uint32_t c = df_lit_code(v);
                if (n == 2u) c |= c << nb;
                df_put(buf, pos, c, n * nb);
            }
            t = n * nb;
        }
        bits += t;
        if (EMIT) pos += t;
    }
    return bits;
}

// sum of the 16 bytes of a lane's group and sum of t * b_t (t = 0..15), by sums of absolute byte differences against
// zero: b1 + 2 b2 + 3 b3 of a word is the byte sum of x >> 8, of x >> 16 and of x >> 24 together
__device__ __forceinline__ void df_byte_sums(const uint32_t (&w)[4], uint32_t &sum, uint32_t &weighted)
{
    sum = 0u;
    weighted = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t s = __builtin_amdgcn_sad_u8(w[q], 0u, 0u);
        sum += s;
        weighted += 4u * q * s;
        weighted = __builtin_amdgcn_sad_u8(w[q] >> 8, 0u, weighted);
        weighted = __builtin_amdgcn_sad_u8(w[q] >> 16, 0u, weighted);
        weighted += w[q] >> 24;
    }
}

// ------------------------------------------------------------------------------------------ one wave per segment
// COUNT (ENCODE = false): seg_bytes[s] = exact bytes of segment s in the output (with the chunk's 2-byte header in its
// first and the 6-byte trailer in its last segment), seg_a[s] = sum of its raw bytes, seg_b[s] = sum of (len - i) b_i,
// both mod 65521.  ENCODE: the segment is assembled in LDS, shifted by the misalignment of its place in `out`, so that
// whole 16-byte lines go out as one store each and only the two ends go byte by byte.  A segment whose recomputed
// size is not the one the offsets were made from (the labels changed between the passes) or that would pass `total`
// is not written at all.
// The loop is over groups of 4 segments per block, so every __syncthreads() is met by all four waves; a wave only
// ever touches its own part of the LDS.
// The 16 bytes of every lane in each round of segment `seg` (zeros past the segment's end and for seg >= n_seg) and the
// element before the segment (0 at a chunk's start).  n_seg is far inside 32 bits: a call's worst case, at least 8
// bytes per segment, fits int32.
template <int ITEM>
__device__ __forceinline__ void df_load(const uint8_t *__restrict__ src, int64_t seg, int64_t n_seg, int64_t L, int64_t S,
                                        int vec_ok, int lane, uint32_t (&w)[DF_ROUNDS][4], uint32_t &prev)
{
#pragma unroll
    for (int r = 0; r < DF_ROUNDS; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[r][q] = 0u;
    prev = 0u;
    if (seg >= n_seg) return;
    const int64_t chunk = (int64_t)((uint32_t)seg / (uint32_t)S), ks = seg - chunk * S;
    const int64_t seg_start = ks * DF_SEG;
    const int slen = (int)(L - seg_start < DF_SEG ? L - seg_start : DF_SEG);
    const uint8_t *base = src + chunk * L + seg_start;
    if (ks > 0) prev = ITEM == 4 ? *reinterpret_cast<const uint32_t *>(base - 4) : (uint32_t)base[-1];
#pragma unroll
    for (int r = 0; r < DF_ROUNDS; ++r) {
        const int boff = r * 1024 + lane * 16;
        if (vec_ok && boff + 16 <= slen) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + boff);
            w[r][0] = v.x; w[r][1] = v.y; w[r][2] = v.z; w[r][3] = v.w;
        } else if (boff < slen) {
            if (ITEM == 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (boff + 4 * j < slen) w[r][j] = *reinterpret_cast<const uint32_t *>(base + boff + 4 * j);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (boff + j < slen) w[r][j >> 2] |= (uint32_t)base[boff + j] << (8 * (j & 3));
            }
        }
    }
}

template <int ITEM, bool ENCODE>
__global__ __launch_bounds__(256) void df_segments_kernel(const uint8_t *__restrict__ src, int64_t n_chunks, int64_t L,
                                                          int64_t S, int vec_ok, int32_t *__restrict__ seg_bytes,
                                                          uint32_t *__restrict__ seg_a, uint32_t *__restrict__ seg_b,
                                                          const int32_t *__restrict__ seg_off,
                                                          const uint32_t *__restrict__ chunk_adler,
                                                          uint8_t *__restrict__ out, int64_t total)
{
    constexpr int FL = 16 / ITEM;
    __shared__ uint32_t s_mask[4][DF_MASK_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t s_buf[ENCODE ? 4 * DF_BUF_LINES * 4 : 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *mask = s_mask[wv];
    uint32_t *buf = ENCODE ? s_buf + wv * DF_BUF_LINES * 4 : s_buf;
    const int64_t n_seg = n_chunks * S;
    uint32_t nw[DF_ROUNDS][4], nprev;                                    // the segment of the NEXT iteration, in flight
    df_load<ITEM>(src, (int64_t)blockIdx.x * 4 + wv, n_seg, L, S, vec_ok, lane, nw, nprev);
    for (int64_t s0 = (int64_t)blockIdx.x * 4; s0 < n_seg; s0 += (int64_t)gridDim.x * 4) {
        const int64_t seg = s0 + wv;
        const bool live = seg < n_seg;                                   // the same in every lane of the wave
        const int64_t chunk = live ? (int64_t)((uint32_t)seg / (uint32_t)S) : 0, ks = live ? seg - chunk * S : 0;
        const int64_t seg_start = ks * DF_SEG;
        const int slen = live ? (int)(L - seg_start < DF_SEG ? L - seg_start : DF_SEG) : 0;
        const uint8_t *base = src + chunk * L + seg_start;
        const uint32_t hdr = ks == 0 ? 2u : 0u, trl = ks == S - 1 ? 6u : 0u;
        int64_t off = 0;
        uint32_t nb_given = 0u, sh = 0u;
        // ---- phase 0: clear this wave's flag mask and as many buffer lines as the segment will take
        for (int i = lane; i < DF_MASK_WORDS; i += 64) mask[i] = 0u;
        if (ENCODE && live) {
            off = seg_off[seg];
            const int64_t nb64 = (int64_t)seg_off[seg + 1] - off;
            nb_given = nb64 > 0 && nb64 <= DF_SEG_MAX_BYTES ? (uint32_t)nb64 : 0u;
            sh = (uint32_t)(reinterpret_cast<uintptr_t>(out + off) & 15u);
            const int lines = (int)((sh + nb_given + 15u) >> 4) + 1;
            for (int i = lane; i < lines && i < DF_BUF_LINES; i += 64)
                reinterpret_cast<uint4 *>(buf)[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        // ---- phase 1: take the segment loaded during the last iteration (kept in registers for the later phases), ask
        // for the next one -- the barriers here wait for LDS only, so it stays in flight while this one is coded --
        // and flag the elements that repeat
        uint32_t w[DF_ROUNDS][4];
#pragma unroll
        for (int r = 0; r < DF_ROUNDS; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[r][q] = nw[r][q];
        uint32_t carry = nprev;                                          // the element before the round's first
        df_load<ITEM>(src, seg + (int64_t)gridDim.x * 4, n_seg, L, S, vec_ok, lane, nw, nprev);
        uint32_t sum_a = 0u, sum_b = 0u;
        if (live) {
#pragma unroll
            for (int r = 0; r < DF_ROUNDS; ++r) {
                const int boff = r * 1024 + lane * 16;
                const int nvalid = min(max((slen - boff) / ITEM, 0), FL);
                const uint32_t last = ITEM == 4 ? w[r][3] : w[r][3] >> 24;
                uint32_t left = __shfl_up(last, 1);
                if (lane == 0) left = carry;
                carry = __shfl(last, 63);
                uint32_t m = 0u;
#pragma unroll
                for (int j = 0; j < FL; ++j) {
                    const uint32_t v = ITEM == 4 ? w[r][j] : (w[r][j >> 2] >> (8 * (j & 3))) & 0xffu;
                    if (j < nvalid && v == left) m |= 1u << j;
                    left = v;
                }
                if (ks == 0 && r == 0 && lane == 0) m &= ~1u;            // a chunk's first element is always literal
                const uint32_t e0 = (uint32_t)(boff / ITEM);
                if (m) atomicOr(&mask[e0 >> 5], m << (e0 & 31u));
                if (!ENCODE) {
                    // bytes past the segment's end are zero here, so their (wrapped) weights do not count
                    uint32_t sb, st;
                    df_byte_sums(w[r], sb, st);
                    sum_a += sb;
                    sum_b += (uint32_t)(slen - boff) * sb - st;
                }
            }
        }
        __syncthreads();
        // ---- phase 2: bits of every lane's tokens, their prefix sum, the segment's size
        uint32_t excl[DF_ROUNDS];
        uint32_t T = 0u;
        if (live) {
#pragma unroll
            for (int r = 0; r < DF_ROUNDS; ++r) {
                const int boff = r * 1024 + lane * 16;
                const int nvalid = min(max((slen - boff) / ITEM, 0), FL);
                const uint32_t c = df_walk<ITEM, false>(w[r], (uint32_t)(boff / ITEM), nvalid, mask, nullptr, 0u);
                uint32_t x = c;
                if (__ballot(c != 0u)) {                                 // rounds inside one long repeat have no token at all
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const uint32_t y = __shfl_up(x, o);
                        if (lane >= o) x += y;
                    }
                }
                excl[r] = T + x - c;
                T += __shfl(x, 63);
            }
        }
        // block header (3 bits), tokens, end of block (7), stored-block header (3), zero bits to the byte, 00 00 FF FF
        const uint32_t body = (3u + T + 10u + 7u) >> 3;
        const uint32_t nb = hdr + body + 4u + trl;
        if (!ENCODE) {
            if (live) {
                unsigned long long a = sum_a, b = sum_b;                 // 64 bits from here: 64 lanes of up to 2^32
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    a += __shfl_down(a, o);
                    b += __shfl_down(b, o);
                }
                if (lane == 0) {
                    seg_bytes[seg] = (int32_t)nb;
                    seg_a[seg] = (uint32_t)(a % DF_MOD);
                    seg_b[seg] = (uint32_t)(b % DF_MOD);
                }
            }
        } else {
            const bool ok = live && nb == nb_given && off + (int64_t)nb <= total;
            if (ok) {
                const uint32_t bit0 = 8u * (sh + hdr);
#pragma unroll
                for (int r = 0; r < DF_ROUNDS; ++r) {
                    const int boff = r * 1024 + lane * 16;
                    const int nvalid = min(max((slen - boff) / ITEM, 0), FL);
                    df_walk<ITEM, true>(w[r], (uint32_t)(boff / ITEM), nvalid, mask, buf, bit0 + 3u + excl[r]);
                }
                if (lane == 0) {
                    if (hdr) { df_put_byte(buf, sh, 0x78u); df_put_byte(buf, sh + 1u, 0x01u); }
                    df_put(buf, bit0, 2u, 3u);                           // BFINAL = 0, BTYPE = 01
                    const uint32_t p = sh + hdr + body;                  // LEN = 0000 stays zero, NLEN = FFFF
                    df_put_byte(buf, p + 2u, 0xffu);
                    df_put_byte(buf, p + 3u, 0xffu);
                    if (trl) {
                        const uint32_t ad = chunk_adler[chunk];
                        df_put_byte(buf, p + 4u, 0x03u);                 // the empty final fixed block: 03 00
                        df_put_byte(buf, p + 6u, ad >> 24);
                        df_put_byte(buf, p + 7u, (ad >> 16) & 0xffu);
                        df_put_byte(buf, p + 8u, (ad >> 8) & 0xffu);
                        df_put_byte(buf, p + 9u, ad & 0xffu);
                    }
                }
            }
            __syncthreads();
            // ---- phase 3: the buffer's bytes [sh, sh + nb) to out + off; line i of the buffer is 16-byte aligned there
            if (ok) {
                uint8_t *g = out + off - sh;
                const uint32_t end = sh + nb;
                const int lines = (int)((end + 15u) >> 4);
                for (int i = lane; i < lines; i += 64) {
                    const uint4 v = reinterpret_cast<const uint4 *>(buf)[i];
                    const uint32_t lo = 16u * i;
                    if (lo >= sh && lo + 16u <= end) {
                        *reinterpret_cast<uint4 *>(g + lo) = v;
                    } else {
                        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int t = 0; t < 16; ++t)
                            if (lo + t >= sh && lo + t < end) g[lo + t] = (uint8_t)(q[t >> 2] >> (8 * (t & 3)));
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ per chunk: offset, Adler-32
// One wave per chunk.  With a = 1 + sum of all bytes and b = n + sum of (n - i) b_i over the chunk's n bytes, segment
// k (its own sums A_k, B_k, `after` bytes behind it) adds A_k to a and B_k + A_k * after to b; all mod 65521, every
// product of two residues inside 32 bits, the sums in 64.
__global__ __launch_bounds__(256) void df_chunks_kernel(const int32_t *__restrict__ seg_off,
                                                        const uint32_t *__restrict__ seg_a,
                                                        const uint32_t *__restrict__ seg_b, int64_t n_chunks, int64_t L,
                                                        int64_t S, uint32_t *__restrict__ chunk_adler,
                                                        int64_t *__restrict__ offsets)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < n_chunks; c += n_waves) {
        unsigned long long a = 0ull, b = 0ull;
        for (int64_t k = lane; k < S; k += 64) {
            const int64_t start = k * DF_SEG;
            const int64_t slen = L - start < DF_SEG ? L - start : DF_SEG;
            const uint32_t after = (uint32_t)((L - start - slen) % DF_MOD);
            const uint32_t A = seg_a[c * S + k];
            a += A;
            b = (b + seg_b[c * S + k] + (unsigned long long)(A * after % DF_MOD)) % DF_MOD;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_down(a, o);
            b += __shfl_down(b, o);
        }
        if (lane == 0) {
            const uint32_t A = (uint32_t)((1ull + a) % DF_MOD);
            const uint32_t B = (uint32_t)(((unsigned long long)(L % DF_MOD) + b) % DF_MOD);
            chunk_adler[c] = (B << 16) | A;
            offsets[c] = (int64_t)seg_off[c * S];
            if (c == n_chunks - 1) offsets[n_chunks] = (int64_t)seg_off[n_chunks * S];
        }
    }
}

// ------------------------------------------------------------------------------------------ entry points
struct DfWork {
    int32_t *seg_bytes, *seg_off, *scantmp;
    uint32_t *seg_a, *seg_b, *chunk_adler;
    int64_t total;
};
static DfWork df_carve(void *work, int64_t n_chunks, int64_t S)
{
    const int64_t n_seg = n_chunks * S;
    EmpCarver c(work);
    DfWork W;
    W.seg_bytes = c.take<int32_t>(n_seg);
    W.seg_off = c.take<int32_t>(n_seg + 1);
    W.seg_a = c.take<uint32_t>(n_seg);
    W.seg_b = c.take<uint32_t>(n_seg);
    W.chunk_adler = c.take<uint32_t>(n_chunks);
    W.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n_seg));
    W.total = c.bytes();
    return W;
}

// shared argument checks; a call's worst case stays inside int32 so that the int32 scan of the segment sizes is exact
#define DF_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                             \
        EMP_REQUIRE(item == 1 || item == 4, what ": item must be 1 (uint8) or 4 (uint32), got %d", item);            \
        EMP_REQUIRE(n_chunks >= 1 && chunk_bytes >= item && chunk_bytes % item == 0,                                 \
                    what ": bad shape (%lld chunks of %lld bytes, item %d)", (long long)n_chunks,                    \
                    (long long)chunk_bytes, item);                                                                   \
        EMP_REQUIRE(chunk_bytes <= 0x70000000LL && n_chunks <= 0x7fffffffLL / df_bound(chunk_bytes),                 \
                    what ": %lld chunks of %lld bytes could take more than 2^31 - 1 bytes; split the slab",          \
                    (long long)n_chunks, (long long)chunk_bytes);                                                    \
    } while (0)

extern "C" int64_t emp_deflate_bound(int64_t chunk_bytes, int item)
{
    EMP_REQUIRE(item == 1 || item == 4, "deflate_bound: item must be 1 (uint8) or 4 (uint32), got %d", item);
    EMP_REQUIRE(chunk_bytes >= item && chunk_bytes % item == 0 && chunk_bytes <= (1LL << 56),
                "deflate_bound: bad chunk size (%lld bytes, item %d)", (long long)chunk_bytes, item);
    return df_bound(chunk_bytes);
}

extern "C" int64_t emp_deflate_work_bytes(int64_t n_chunks, int64_t chunk_bytes, int item)
{
    DF_REQUIRE_SHAPE("deflate_work_bytes");
    return df_carve(nullptr, n_chunks, emp_cdiv(chunk_bytes, DF_SEG)).total;
}

template <bool ENCODE>
static int df_launch(const void *src, int item, int64_t n_chunks, int64_t L, const DfWork &W, uint8_t *out,
                     int64_t total, hipStream_t st)
{
    const int64_t S = emp_cdiv(L, DF_SEG);
    const uint8_t *p = reinterpret_cast<const uint8_t *>(src);
    // 16-byte loads need every chunk (and with it every segment) to start on a 16-byte address
    const int vec_ok = (reinterpret_cast<uintptr_t>(src) % 16 == 0 && L % 16 == 0) ? 1 : 0;
    const int grid = emp_grid(n_chunks * S * 64, 256, 2048);
    if (item == 4)
        EMP_LAUNCH((df_segments_kernel<4, ENCODE>), grid, 256, st, p, n_chunks, L, S, vec_ok, W.seg_bytes, W.seg_a,
                   W.seg_b, W.seg_off, W.chunk_adler, out, total);
    else
        EMP_LAUNCH((df_segments_kernel<1, ENCODE>), grid, 256, st, p, n_chunks, L, S, vec_ok, W.seg_bytes, W.seg_a,
                   W.seg_b, W.seg_off, W.chunk_adler, out, total);
    return EMP_OK;
}

extern "C" int emp_deflate_count(const void *src, int item, int64_t n_chunks, int64_t chunk_bytes, void *work,
                                 int64_t work_bytes, int64_t *offsets, void *stream)
{
    EMP_REQUIRE(src && work && offsets, "deflate_count: null pointer");
    DF_REQUIRE_SHAPE("deflate_count");
    EMP_REQUIRE(reinterpret_cast<uintptr_t>(src) % (uintptr_t)item == 0, "deflate_count: misaligned labels");
    const int64_t S = emp_cdiv(chunk_bytes, DF_SEG);
    DfWork W = df_carve(work, n_chunks, S);
    EMP_REQUIRE(work_bytes >= W.total, "deflate_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)W.total);
    hipStream_t st = emp_stream(stream);
    int rc = df_launch<false>(src, item, n_chunks, chunk_bytes, W, nullptr, 0, st);
    if (rc != EMP_OK) return rc;
    rc = emp_exclusive_scan_i32(W.seg_bytes, n_chunks * S, W.seg_off, W.scantmp, stream);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(df_chunks_kernel, emp_grid(n_chunks * 64, 256, 2048), 256, st, W.seg_off, W.seg_a, W.seg_b, n_chunks,
               chunk_bytes, S, W.chunk_adler, offsets);
    return EMP_OK;
}

extern "C" int emp_deflate_encode(const void *src, int item, int64_t n_chunks, int64_t chunk_bytes, void *work,
                                  int64_t work_bytes, int64_t total, uint8_t *out, int64_t out_bytes, void *stream)
{
    EMP_REQUIRE(src && work && out, "deflate_encode: null pointer");
    DF_REQUIRE_SHAPE("deflate_encode");
    EMP_REQUIRE(reinterpret_cast<uintptr_t>(src) % (uintptr_t)item == 0, "deflate_encode: misaligned labels");
    const int64_t S = emp_cdiv(chunk_bytes, DF_SEG);
    DfWork W = df_carve(work, n_chunks, S);
    EMP_REQUIRE(work_bytes >= W.total, "deflate_encode: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)W.total);
    EMP_REQUIRE(total >= 0 && total <= n_chunks * df_bound(chunk_bytes),
                "deflate_encode: total = %lld is not the byte total of %lld chunks of %lld bytes", (long long)total,
                (long long)n_chunks, (long long)chunk_bytes);
    EMP_REQUIRE(out_bytes >= total, "deflate_encode: output too small (%lld < %lld)", (long long)out_bytes,
                (long long)total);
    return df_launch<true>(src, item, n_chunks, chunk_bytes, W, out, total, emp_stream(stream));
}
