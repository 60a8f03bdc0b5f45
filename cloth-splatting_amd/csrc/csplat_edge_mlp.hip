// csplat_edge_mlp.hip -- the WHOLE edge MLP of an InteractionNetwork layer in one launch (rollout / inference, BASELINE configs[3]):
//
//   msg[e] = LayerNorm( W3 relu( W2 relu( alpha * We e0[e] + b0 + xa[dst[e]] + xb[src[e]] ) + b2 ) + b3 )
//
// = /root/reference/meshnet/graph_network.py:178-199 (`message`: edge_fn(cat[x_i, x_j, e]) with the first Linear cut into its three
// column blocks, the x_i / x_j blocks applied at node level: xa = x Wi^T (+ bias rides in b0 here), xb = x Wj^T) for edge features
// alpha * e0 (every layer doubles its edge features, SURVEY F7: alpha = 2^l).
//
// Rounds 1-4 ran this as three csplat_linear128 launches, each a full [E,128] HBM round trip (307 MB per launch at E = 300k: 75-97 us
// each, memory-paced: 235-245 us per layer).  Here the two inner [rows,128] activations never leave the chip: traffic per layer is 154 MB
// in + 154 MB out (+ the L2-resident gathers), and the kernel is paced by its matrix and vector instruction issue.
//
// Design (gfx950): WEIGHTS RESIDENT IN REGISTERS.  One 4-wave workgroup per CU, one wave per SIMD (the whole 512-register file each);
// wave j owns output features 32j .. 32j + 31 of ALL THREE layers.  The products run on the 32x32x16 MFMA with both operands cut into
// 16-bit pieces, fp32 accumulation, TRANSPOSED: A operand = weight rows (output features), B operand = activations (lane = edge row), so
// a lane ends a layer holding 32 features of its own row.  The weights' pieces are MFMA A operands loaded ONCE per launch -- straight
// into the accumulation half of the register file, where inline-asm MFMAs read them (values that only ever meet "a" constraints: the
// allocator never moves them).  What travels through LDS is the ACTIVATIONS, already cut into pieces by whoever produced them: a 32-row
// tile is [piece][32 rows][128 + 8] x 16 bit.  Two tiles per workgroup are in flight ONE LAYER APART (slots A and B); a phase = the NS
// MFMAs of one tile's layer on one accumulation chain, and in the gaps between those MFMAs ride the OTHER tile's epilogue (ReLU + cut
// into pieces + LDS writes, or LayerNorm) and the loaders of the next tiles (edge rows, gathered node rows: whole rows per instruction,
// half-wave per row; G = s (b0 + xa[dst] + xb[src]) is what layer 1's accumulators START from, as the other layers' start from
// their bias).  One wave per SIMD means nothing hides behind another wave: a gap hides ~5 single-issue instructions, so every side task
// is a numbered list of 1-4-instruction operations dealt evenly over a range of gaps (ER_SPREAD), and scheduling barriers pin the order.
// LayerNorm's statistics cross the four waves through LDS ((sum, M2) per wave, combined by the parallel-variance formula).  One barrier
// per phase; rows out as 16 bytes per lane by buffer stores (rows past E are dropped by the bounds check: no branch).
// Contraction order: position pos = 64h + 8st + i of an activation row is what lane-half h feeds into step st as element i.  Layer 1:
// pos = column of e0.  Layers 2, 3: the producing wave j' writes its lane's 16 accumulator registers of row n contiguously, pos = 32j'
// + 16h' + r <-> feature 32j' + 8(r >> 2) + 4h' + (r & 3); the permutation is applied to the packed weights (er_src_col).
//
// Two arithmetic modes (csplat_gnn_edge_mlp3_mode; Piece<F16> holds their piece arithmetic for this kernel, both packers and PieceChain<F16>,
// which the node update k_node_update_b3 and the rows chain k_rows_chain further down are written on):
//   0  two fp16 pieces per operand (x = h1 + h2 to 2^-22 |x|), three products per step (h1 h1 + h1 h2 + h2 h1): 24 MFMAs per tile-layer.
//      fp16 has 5 exponent bits, so the values are kept where they are representable: the launch's max |e0| (csplat_absmax, once per
//      rollout step: e0 is the same for all layers) gives the power of two cs that brings the edge rows to max in [8, 16), and ALL the
//      arithmetic runs multiplied by s = cs / alpha (exact; ReLU is homogeneous, LayerNorm takes s^2 eps).  An element below 2^-3 of
//      fp16's normal range keeps an ABSOLUTE error of 2^-25 in the scaled units, and a row's LayerNorm divides that by the row's own
//      size: what a row loses depends on how far its inner activations sit below the LAUNCH's scale (max |e0| x alpha: alpha multiplies
//      the edge term only, so a row whose edge features are small or zero -- its node terms s (b0 + xa + xb) alone -- sits alpha times
//      lower).  Per row, in units of max(max_j |out|, 1), against fp64, from the float64 model of this arithmetic (tests/edge_mlp_ref.py,
//      table in tests/test_edge_mlp_cpu.py; fp32 itself: 5e-7):
//        rows within 2^6 of the launch's scale (ordinary, one-hot, zero and 2^-20 rows at alpha <= 64; one edge row 2^6 above the
//        others or e0_absmax overstated by 2^6 at alpha <= 1)                                                        4e-7 .. 9e-7
//        the same with weight elements down to 1e-3 of their matrix' largest: 4e-7 at alpha <= 1, 1.7e-6 at alpha 64
//        2^12 (one edge row 2^12 above the others: THEIR rows; or 2^6 at alpha 64)                                   3e-5 .. 5e-5
//        2^14 (alpha 16384 on rows without edge features) 1e-4; 2^20 and beyond: 1e-2 .. O(1)
//      The largest row of a launch always keeps 2e-7 .. 1e-6.  Upwards: an inner activation beyond 65504 in the scaled units (2^12 above the
//      edge rows' scale; an understated e0_absmax, or edge rows far BELOW O(1) node terms -- max |e0| = 1e-6 puts s at 2^23) leaves fp16's
//      range and shows as a NaN row, never as a wrong finite one.  LayerNorm'd latents and trained / initialised MLPs sit in the middle.
//   1  three bf16 pieces per operand, the six products that matter: 48 MFMAs per tile-layer, fp32's exponent range, no scaling beyond
//      1 / alpha.  7e-7 against fp64 on anything fp32 can hold.
//
// MEASURED (round 5, E = 300k, tools/bench_edge_mlp3.py / edge_mlp3_stamps.py / ab_edge_mlp3_rollout.py): see DESIGN.md section 6.
// History of the design (docs/HISTORY.md): four versions with the weights staged through LDS (one image, eight waves in lockstep) never
// beat the three launches; the bare MFMA pipeline of THIS design runs at 1,736 cycles per 48-MFMA phase (floor 1,536), the chip's clock
// under it at ~1.7 GHz.
#include "csplat_common.h"
#include "csplat_device.h"
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#ifndef EM_SKIP
#define EM_SKIP 0      /* timing experiments (tools/edge_mlp3_skip_ab.sh): side tasks left out of the phases -- results wrong */
#endif

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short el16;              // a 16-bit piece in LDS (bf16 or fp16 by mode)
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));

constexpr int EM_N = 128;                 // layer width
constexpr int EM_STRIDE = 136;            // 16-bit elements per activation row in LDS (272 B: conflict-free 16-byte operand reads)
constexpr int ER_TILE_P = 32 * EM_STRIDE;                 // elements of one piece of one 32-row tile
constexpr int ER_GSTRIDE = 132;                           // floats per G row (528 B: conflict-free 16-byte accesses, lane = row)
constexpr size_t ER_G_BYTES = (size_t)64 * ER_GSTRIDE * 4;        // 33,792
constexpr size_t ER_S_BYTES = (size_t)2 * 32 * 4 * 8;     // LayerNorm partials [slot][row 32][wave 4] (sum, M2)
constexpr size_t ER_T_BYTES = (size_t)4 * EM_N * 4;       // b1, b2, gamma, beta

// The 16-bit piece arithmetic of one mode (header): x = p[0] + p[1] (+ p[2]), each piece what its format holds of the remainder the pieces
// before it left.  All three piece kernels and both packers take their pieces from here.
template <bool F16> struct Piece {
    static constexpr int NP = F16 ? 2 : 3;                // pieces per operand
    static constexpr int NPROD = F16 ? 3 : 6;             // products per k-step
    static constexpr float SC = F16 ? 0.0625f : 1.f, ISC = F16 ? 16.f : 1.f;      // PieceChain's fixed scale and its inverse (the edge kernel has its own)
    // two values -> one dword of 16-bit pieces (round to nearest even), and the two pieces back as floats
    static __device__ __forceinline__ unsigned pk(float lo, float hi) {
        if (F16) { h16x2 v; v[0] = (_Float16)lo; v[1] = (_Float16)hi; return __builtin_bit_cast(unsigned, v); }
        bf16x2 v; v[0] = (__bf16)lo; v[1] = (__bf16)hi;
        return __builtin_bit_cast(unsigned, v);
    }
    static __device__ __forceinline__ float lo_f(unsigned q) {
        if (F16) return (float)__builtin_bit_cast(h16x2, q)[0];
        return __uint_as_float(q << 16);
    }
    static __device__ __forceinline__ float hi_f(unsigned q) {
        if (F16) return (float)__builtin_bit_cast(h16x2, q)[1];
        return __uint_as_float(q & 0xffff0000u);
    }
    // one value -> its NP pieces, one at a time (the packers' form)
    static __device__ __forceinline__ void split(float x, el16 (&p)[3]) {
#pragma unroll
        for (int q = 0; q < NP; q++) {
            if (F16) { const _Float16 v = (_Float16)x; p[q] = __builtin_bit_cast(el16, v); x -= (float)v; }
            else { const __bf16 v = (__bf16)x; p[q] = __builtin_bit_cast(el16, v); x -= (float)v; }
        }
    }
};

template <bool F16> struct ErCfg {
    static constexpr int NP = Piece<F16>::NP, NPROD = Piece<F16>::NPROD;
    static constexpr int NS = 8 * NPROD;                  // MFMAs (and gaps) per phase
    static constexpr int NW = 3 * NP * 8;                 // A operands per wave
    static constexpr int XT = NP * ER_TILE_P;             // elements of one tile buffer
    static constexpr size_t X_BYTES = (size_t)4 * XT * 2; // [slot 2][buffer 2]: 104,448 / 69,632
    static constexpr bool ROWS_VIA_LDS = F16;             // finished rows cross LDS and leave as whole rows (room for it with two pieces only)
    static constexpr size_t Y_BYTES = ROWS_VIA_LDS ? ER_G_BYTES : 0;      // [slot 2][32][ER_GSTRIDE] floats
    static constexpr size_t LDS_BYTES = X_BYTES + ER_G_BYTES + ER_S_BYTES + ER_T_BYTES + Y_BYTES;
    static constexpr size_t IMAGE_BYTES = (size_t)4 * NW * 64 * 16;      // [wave][layer][piece][step][lane] x 16 B: 294,912 / 196,608
};

__host__ __device__ inline int er_src_col(int layer, int pos) {
    if (layer == 0) return pos;
    const int j = pos >> 5, h = (pos >> 4) & 1, r = pos & 15;
    return 32 * j + 8 * (r >> 2) + 4 * h + (r & 3);
}

// What both packers do for a lane: the 8 contraction elements (positions 64h + 8st .. + 7, through er_src_col of `layer`) of one output
// feature's weight row (W + row_off), cut into pieces -> the NP 16-byte MFMA A operands op[0 .. NP - 1]
template <bool F16>
__device__ __forceinline__ void pack_operands(const float *__restrict__ W, size_t row_off, int layer, int h, int st, i32x4 (&op)[3]) {
    el16 p[3][8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        el16 e[3];
        Piece<F16>::split(W[row_off + er_src_col(layer, 64 * h + 8 * st + i)], e);
#pragma unroll
        for (int q = 0; q < Piece<F16>::NP; q++) p[q][i] = e[q];
    }
#pragma unroll
    for (int q = 0; q < Piece<F16>::NP; q++) op[q] = *reinterpret_cast<const i32x4 *>(p[q]);
}

template <bool F16>
__global__ __launch_bounds__(64) void k_edge_mlp3r_pack(const float *__restrict__ W0, int ld0, const float *__restrict__ W1, int ld1,
                                                        const float *__restrict__ W2, int ld2, i32x4 *__restrict__ img) {
    // block = (wave j, layer l, step st); lane (m, h): the 8 contraction elements of output feature 32j + m it feeds into step st
    constexpr int NP = ErCfg<F16>::NP;
    const int st = blockIdx.x & 7, l = (blockIdx.x >> 3) % 3, j = blockIdx.x / 24;
    const int lane = threadIdx.x, m = lane & 31, h = lane >> 5;
    const float *W = l == 0 ? W0 : (l == 1 ? W1 : W2);
    const int ld = l == 0 ? ld0 : (l == 1 ? ld1 : ld2);
    i32x4 op[3];
    pack_operands<F16>(W, (size_t)(32 * j + m) * ld, l, h, st, op);
#pragma unroll
    for (int q = 0; q < NP; q++) img[((size_t)j * ErCfg<F16>::NW + (l * NP + q) * 8 + st) * 64 + lane] = op[q];
}

// Every ReLU here is relu_keep_nan (csplat_common.h: `x < 0.f ? 0.f : x`, a NaN passes).  A value that left fp16's range turns into NaN one layer later (pieces Inf and -Inf),
// which a fmaxf ReLU would then launder into finite garbage: measured, a first-layer weight of 3e4 gave finite rows with a relative error
// of 1.2.  With this form an overflow anywhere reaches the output as NaN rows: visible, never silent.

__device__ __forceinline__ float pair_sum(float v) {      // v of lane (n, 0) + v of lane (n, 1), in both lanes
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(sw[0]) + __int_as_float(sw[1]);
}

// max |x| over n floats -> *out (bits of a non-negative float order as integers: one atomic per workgroup); *out zeroed by the caller
__global__ __launch_bounds__(256) void k_absmax(int64_t n4, const float4 *__restrict__ x, unsigned *__restrict__ out) {
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = x[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    __shared__ float sm[4];
    block_stash(sm, wave_max(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned b = __float_as_uint(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])));
        if (b > *reinterpret_cast<volatile unsigned *>(out)) atomicMax(out, b);      // (a stale read costs an extra atomic, never the result)
    }
}

template <bool F16, int MODE>      // MODE 0: message rows out; 1: messages summed per destination, pieces out; 2: narrow input rows, no gathers
__global__ __launch_bounds__(256) void k_edge_mlp3r(int64_t M, const float *__restrict__ e0, float alpha, const float *__restrict__ e0_absmax,
                                                    const float *__restrict__ xa, const int64_t *__restrict__ ia,
                                                    const float *__restrict__ xb, const int64_t *__restrict__ ib,
                                                    const i32x4 *__restrict__ wimg, const float *__restrict__ b0,
                                                    const float *__restrict__ b1, const float *__restrict__ b2,
                                                    const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                    float *__restrict__ out, const int *__restrict__ group_piece0, float *__restrict__ pieces,
                                                    int in_cols, unsigned long long *__restrict__ stamps) {
    constexpr bool AGG = MODE == 1, NARROW = MODE == 2;
    static_assert(!AGG || ErCfg<F16>::ROWS_VIA_LDS, "the fused aggregation reads the finished tile from LDS");
    typedef ErCfg<F16> C;
    constexpr int NP = C::NP, NS = C::NS;
    extern __shared__ char s_mem[];
    el16 *const sX = reinterpret_cast<el16 *>(s_mem);                                         // [slot 2][buffer 2] tiles of NP pieces
    float *const sG = reinterpret_cast<float *>(s_mem + C::X_BYTES);                          // [slot 2][32][ER_GSTRIDE]
    float2 *const sS = reinterpret_cast<float2 *>(s_mem + C::X_BYTES + ER_G_BYTES);           // [slot 2][32][wave 4] (sum, M2)
    float *const sT = reinterpret_cast<float *>(s_mem + C::X_BYTES + ER_G_BYTES + ER_S_BYTES);      // b1, b2, gamma, beta
    float *const sY = reinterpret_cast<float *>(s_mem + C::X_BYTES + ER_G_BYTES + ER_S_BYTES + ER_T_BYTES);      // finished rows [slot 2][32][ER_GSTRIDE]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, h = lane >> 5;

    int stamp_at = 0;                         // (measurement hook, csplat_debug_stamps / tools/edge_mlp3_stamps.py)
    auto stamp = [&]() {
        if (stamps && w == 0 && stamp_at < 64) {
            const unsigned long long t = __builtin_readcyclecounter();
            if (lane == 0) stamps[(size_t)blockIdx.x * 64 + stamp_at] = t;
            stamp_at++;
        }
    };

    // ---- this wave's 32 output features of the three layers: 3 x NP x 8 MFMA A operands (72 = 288 registers with three bf16 pieces, 48 =
    // 192 with two fp16 pieces), for the whole launch.  Up to 64 of them are OWNED through "a" constraints (loaded straight into
    // accumulation registers, read there by the MFMAs: the allocator never sees them as something to move), the rest live with the
    // loop's own values in the architectural half.
    i32x4 Wa[64], Wv[8];
#pragma unroll
    for (int id = 0; id < C::NW; id++) {
        const i32x4 *src = wimg + ((size_t)w * C::NW + id) * 64 + lane;      // image: [wave][layer][piece][step][lane]
        if (id < 64) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(Wa[id]) : "v"(src) : "memory");
        else Wv[id - 64] = *src;
    }
    // the scale everything runs in.  bf16 pieces have fp32's exponent range: values run divided by alpha, nothing else.  fp16 pieces
    // do not: the edge rows are brought to max |e0| in [8, 16) first (e0_absmax: the launch's max |e0|, left on the device by
    // csplat_absmax), so that what the layers hand on sits in the middle of fp16's range (header)
    float cs = 1.f;
    if (F16) {
        const float m = e0_absmax ? *e0_absmax : 1.f;
        int ex = 0;
        if (m > 0.f && m < 3.0e38f) (void)frexpf(m, &ex);      // m = f 2^ex, f in [0.5, 1)
        // (a tiny or denormal max |e0| would make 2^(4 - ex) overflow to Inf and the whole launch NaN -- ADVICE r5; below 2^-96 the rows
        //  are left smaller than [8, 16): what they contribute next to the node-level terms is below fp32 rounding anyway)
        ex = ex < -96 ? -96 : (ex > 100 ? 100 : ex);
        cs = ldexpf(1.f, 4 - ex);
    }
    const float inv_alpha = cs / alpha;       // (a power of two: every product with it is exact)
    for (int t = threadIdx.x; t < 4 * EM_N; t += 256)
        sT[t] = t < EM_N ? b1[t] * inv_alpha : (t < 2 * EM_N ? b2[t - EM_N] * inv_alpha : (t < 3 * EM_N ? gamma[t - 2 * EM_N] : beta[t - 3 * EM_N]));
    eps *= inv_alpha * inv_alpha;             // (everything runs multiplied by cs / alpha: see the side work)
    float4 b0v = *reinterpret_cast<const float4 *>(b0 + 4 * n);       // (loader layout: half-wave per row, lane n <-> columns 4n .. 4n + 3)
    b0v.x *= inv_alpha; b0v.y *= inv_alpha; b0v.z *= inv_alpha; b0v.w *= inv_alpha;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // (the asm loads are not in the compiler's books)
    __builtin_amdgcn_sched_barrier(0);

    // one product: acc += W[id] x b.  Accumulate chain: an MFMA's D taken whole as the next one's C needs no wait states; B comes from
    // LDS reads (counted by the compiler); the chain's readers run a barrier later
    auto mfma = [&](int id, const i32x4 &b, f32x16 &acc) __attribute__((always_inline)) {
        if (F16) {
            if (id < 64) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(Wa[id & 63]), "v"(b));
            else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(Wv[id & 7]), "v"(b));
        } else {
            if (id < 64) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(Wa[id & 63]), "v"(b));
            else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(Wv[id & 7]), "v"(b));
        }
    };
    constexpr auto pk = Piece<F16>::pk;
    constexpr auto lo_f = Piece<F16>::lo_f, hi_f = Piece<F16>::hi_f;

    // =================== side work, cut into operations of 1-4 instructions that ride in the gaps between MFMAs.  One wave per SIMD: a gap
    // hides ~5 single-issue instructions, the sixth costs its full price -- so every task is a numbered list of small operations and
    // spread() deals a task's list evenly over a range of a phase's 48 gaps.
    // Everything below works on values scaled by s = cs / alpha (a power of two: exact): layer 1 accumulates We (cs e0) + s (b0 + xa + xb),
    // the biases of layers 2 and 3 are parked multiplied by s, and LayerNorm runs with s^2 eps -- (z - m) / sqrt(v + eps) =
    // (sz - sm) / sqrt(s^2 v + s^2 eps) -- so no ReLU carries a multiplication.
    // (a macro: the per-gap trip count must be a literal for the loop to unroll before the gap index is known)
#define ER_SPREAD(k, S0, S1, N, OP)                                                                                   \
    do {                                                                                                              \
        if ((k) >= (S0) && (k) < (S1)) {                                                                              \
            const int a_ = ((k) - (S0)) * (N) / ((S1) - (S0)), b_ = ((k) + 1 - (S0)) * (N) / ((S1) - (S0));           \
            _Pragma("unroll") for (int d_ = 0; d_ < ((N) + (S1) - (S0) - 1) / ((S1) - (S0)); d_++) {                  \
                const int m = a_ + d_;                                                                                \
                if (m < b_) { OP; }                                                                                   \
            }                                                                                                         \
        }                                                                                                             \
    } while (0)
    auto opaque = [&](unsigned &q) __attribute__((always_inline)) { asm volatile("" : "+v"(q)); };      // (keeps a packed pair ONE conversion: see pk)
    // ---- ReLU(acc) -> the next layer's NP pieces, positions 32w + 16h .. + 15 of row n.  Per value pair (max, max, pack), then per further
    // piece (low -) (high -) (pack); NP x 16-byte writes after pairs 0-3 and after pairs 4-7
    constexpr int RELU_PAIR = 3 * NP - 2, RELU_HALF = 4 * RELU_PAIR + NP, RELU_OPS = 2 * RELU_HALF;
    float rx0 = 0.f, rx1 = 0.f;
    unsigned P[NP][4], rq = 0;
    auto relu_op = [&](int m, const f32x16 &acc, el16 *Xtile) __attribute__((always_inline)) {
        const int half = m / RELU_HALF, mm = m % RELU_HALF;
        if (mm < 4 * RELU_PAIR) {
            const int jj = mm / RELU_PAIR, j = 4 * half + jj, o = mm % RELU_PAIR;
            if (o == 0) { rx0 = relu_keep_nan(acc[2 * j]); rx1 = relu_keep_nan(acc[2 * j + 1]); rq = pk(rx0, rx1); opaque(rq); P[0][jj] = rq; }
            else if (o % 3 == 1) rx0 -= lo_f(rq);
            else if (o % 3 == 2) rx1 -= hi_f(rq);
            else { rq = pk(rx0, rx1); if (o != RELU_PAIR - 1) opaque(rq); P[o / 3][jj] = rq; }
        } else {
            const int p = mm - 4 * RELU_PAIR;
            el16 *dst = Xtile + (size_t)p * ER_TILE_P + (size_t)n * EM_STRIDE + 32 * w + 16 * h + 8 * half;
            *reinterpret_cast<uint4 *>(dst) = make_uint4(P[p][0], P[p][1], P[p][2], P[p][3]);
        }
    };
    // ---- LayerNorm, first half: this wave's (sum, M2 about its own mean) of the 32 features it holds of row n: 14 operations
    constexpr int LNP_OPS = 14;
    float ln_s = 0.f, ln_mj = 0.f, ln_m2 = 0.f;
    auto lnp_op = [&](int m, const f32x16 &acc, float2 *srow) __attribute__((always_inline)) {
        if (m < 4) {
            const float t = (acc[4 * m] + acc[4 * m + 1]) + (acc[4 * m + 2] + acc[4 * m + 3]);
            ln_s = m == 0 ? t : ln_s + t;
        } else if (m == 4) {
            ln_s = pair_sum(ln_s);
            ln_mj = ln_s * (1.f / 32.f);
        } else if (m < 13) {
            const int q = m - 5;              // two values each
            float t = q == 0 ? 0.f : ln_m2;
#pragma unroll
            for (int r = 2 * q; r < 2 * q + 2; r++) { const float d = acc[r] - ln_mj; t = fmaf(d, d, t); }
            ln_m2 = t;
        } else {
            ln_m2 = pair_sum(ln_m2);
            srow[w] = make_float2(ln_s, ln_m2);      // (both half-waves write the same pair)
        }
    };
    // ---- second half: the four waves' partials combined (parallel-variance formula), normalise, scale / shift, 4 x 16 bytes out: 18 operations
    constexpr int LNF_OPS = 18;
    const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(M * 512), 0x00020000);      // (rows past M: dropped)
    const int st_lane = n * 512 + (32 * w + 4 * h) * 4;
    float4 lf_u0, lf_u1, lf_ga, lf_be;
    float lf_mean = 0.f, lf_m2 = 0.f, lf_rstd = 0.f, lf_nm = 0.f, lf_y[4];
    auto lnf_op = [&](int m, const f32x16 &acc, const float2 *srow, unsigned tile_off, float *Yt) __attribute__((always_inline)) {
        if (m == 0) {
            lf_u0 = *reinterpret_cast<const float4 *>(srow); lf_u1 = *reinterpret_cast<const float4 *>(srow + 2);
        } else if (m == 1) {
            lf_mean = ((lf_u0.x + lf_u0.z) + (lf_u1.x + lf_u1.z)) * (1.f / EM_N);
        } else if (m == 2) {
            lf_m2 = (lf_u0.y + lf_u0.w) + (lf_u1.y + lf_u1.w);
            const int f = 32 * w + 4 * h;
            lf_ga = *reinterpret_cast<const float4 *>(sT + 2 * EM_N + f); lf_be = *reinterpret_cast<const float4 *>(sT + 3 * EM_N + f);
        } else if (m == 3) {
            const float d0 = fmaf(lf_u0.x, 1.f / 32.f, -lf_mean), d1 = fmaf(lf_u0.z, 1.f / 32.f, -lf_mean);
            lf_y[0] = d0 * d0; lf_y[0] = fmaf(d1, d1, lf_y[0]);
        } else if (m == 4) {
            const float d2 = fmaf(lf_u1.x, 1.f / 32.f, -lf_mean), d3 = fmaf(lf_u1.z, 1.f / 32.f, -lf_mean);
            lf_y[0] = fmaf(d2, d2, lf_y[0]); lf_y[0] = fmaf(d3, d3, lf_y[0]);
        } else if (m == 5) {
            lf_m2 = fmaf(32.f, lf_y[0], lf_m2);
            lf_rstd = __builtin_amdgcn_rsqf(fmaf(lf_m2, 1.f / EM_N, eps));
            lf_nm = -lf_mean * lf_rstd;
        } else {
            const int q = (m - 6) / 3, part = (m - 6) % 3;
            if (part == 0) {
#pragma unroll
                for (int i = 0; i < 4; i++) lf_y[i] = fmaf(acc[4 * q + i], lf_rstd, lf_nm);
            } else if (part == 1) {
                lf_y[0] = fmaf(lf_y[0], lf_ga.x, lf_be.x); lf_y[1] = fmaf(lf_y[1], lf_ga.y, lf_be.y);
                lf_y[2] = fmaf(lf_y[2], lf_ga.z, lf_be.z); lf_y[3] = fmaf(lf_y[3], lf_ga.w, lf_be.w);
                if (q < 3) {
                    const int f = 32 * w + 8 * (q + 1) + 4 * h;
                    lf_ga = *reinterpret_cast<const float4 *>(sT + 2 * EM_N + f); lf_be = *reinterpret_cast<const float4 *>(sT + 3 * EM_N + f);
                }
            } else {
                if (C::ROWS_VIA_LDS) {
                    *reinterpret_cast<float4 *>(Yt + (size_t)n * ER_GSTRIDE + 32 * w + 8 * q + 4 * h) = make_float4(lf_y[0], lf_y[1], lf_y[2], lf_y[3]);
                } else {      // 16 bytes of the lane's own row: 32 lines per instruction
                    i32x4 v;
                    v[0] = __float_as_int(lf_y[0]); v[1] = __float_as_int(lf_y[1]); v[2] = __float_as_int(lf_y[2]); v[3] = __float_as_int(lf_y[3]);
                    __builtin_amdgcn_raw_buffer_store_b128(v, r_out, st_lane + tile_off + 32 * q, 0, 0);
                }
            }
        }
    };
    // ---- (ROWS_VIA_LDS) the finished tile leaves as WHOLE rows, a phase after LayerNorm parked it: a wave takes rows 8w .. 8w + 7, two per
    // instruction -- 8 cache lines per store instead of the 32 a lane-owns-its-row store touches (the L1 / address unit prices a memory
    // instruction by its lines, and the rows out were the dearest thing in the kernel: tools/edge_mlp3_skip_ab.sh).  8 operations
    const int ld_lane = (8 * w + h) * 512 + 16 * n;       // (loader / whole-row layout: half-wave per row, 16 bytes per lane)
    float4 ro[2];
    auto rows_out_op = [&](int m, const float *Yt, unsigned tile_off) __attribute__((always_inline)) {
        constexpr int RDK[8] = {0, 1, -1, 2, -1, 3, -1, -1}, STK[8] = {-1, -1, 0, -1, 1, -1, 2, 3};
        if (RDK[m] >= 0) ro[RDK[m] & 1] = *reinterpret_cast<const float4 *>(Yt + (size_t)(8 * w + 2 * RDK[m] + h) * ER_GSTRIDE + 4 * n);
        if (STK[m] >= 0 && !(EM_SKIP & 64))
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, ro[STK[m] & 1]), r_out, ld_lane + tile_off + 1024 * STK[m], 0, 0);
    };
    // ---- (AGG) ... or does not leave at all: the tile's rows are in DESTINATION order (the caller permuted the edge list), so what the
    // network needs of them -- their sum per destination node, /root/reference/meshnet/graph_network.py:201-222 (aggr = 'add') -- is a sum
    // over runs of consecutive rows.  A wave sums ITS 8 rows (lane <-> two columns) run by run and writes one 512-byte "piece" per run:
    // pieces are cut where the destination changes and every 8 rows, numbered in row order (group_piece0[g] = first piece of rows 8g ..
    // 8g + 7, prepared once per graph), so each piece has exactly one writer and the caller adds a node's few consecutive pieces in a
    // fixed order: deterministic, no atomics, and ~E / 8 + N rows of traffic instead of E written here and E read by the segmented sum.
    // The run structure is wave-uniform: the 8 destinations and the piece base are fetched by two small vector loads and spread with
    // v_readlane (SCALAR loads -- out-of-order returns, one counter with LDS -- make every LDS wait a wait for them too: measured +17 % on
    // the kernel when the gather indices went that way).  9 operations
    const __amdgpu_buffer_rsrc_t r_pc = __builtin_amdgcn_make_buffer_rsrc(pieces, 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_gp = __builtin_amdgcn_make_buffer_rsrc((void *)group_piece0, 0, AGG ? (int)(((M + 7) / 8) * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_dst = __builtin_amdgcn_make_buffer_rsrc((void *)ia, 0, (int)(M * 8), 0x00020000);
    int ag_d[8], ag_nv = 0, ag_p = 0;
    int2 ag_lA = make_int2(0, 0), ag_lB = make_int2(0, 0);      // per slot: (the 8 destinations in lanes 0-7, the piece base), requested a phase ahead
    float2 ag_acc = make_float2(0.f, 0.f), ag_y = make_float2(0.f, 0.f);
    auto agg_load_op = [&](int tile, int2 &l) __attribute__((always_inline)) {
        const int64_t row0 = (int64_t)tile * 32 + 8 * w;
        l.x = __builtin_amdgcn_raw_buffer_load_b32(r_dst, (int)(row0 * 8) + (lane & 7) * 8, 0, 0);      // (past the end: 0, unused)
        l.y = __builtin_amdgcn_raw_buffer_load_b32(r_gp, (int)(row0 >> 3) * 4, 0, 0);
    };
    // operation 0: the run structure to the scalar side, the first row requested; operation r + 1: row r added (the next one requested
    // first: a row's LDS read is a whole operation ahead of its use), its run closed -- one 512-byte store -- when the destination changes.
    // (Branch-free, every row storing and the stores that close no run aimed out of bounds: slower, 122-127 against 118 us -- a dropped
    // store is still a memory instruction.)
    auto agg_op = [&](int m, const float *Yt, int tile, const int2 &l) __attribute__((always_inline)) {
        const float *yrow = Yt + (size_t)(8 * w) * ER_GSTRIDE + 2 * lane;
        if (m == 0) {
            const int64_t row0 = (int64_t)tile * 32 + 8 * w, left = M - row0;
            ag_nv = left < 0 ? 0 : (left > 8 ? 8 : (int)left);
            ag_acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < 8; q++) ag_d[q] = __builtin_amdgcn_readlane(l.x, q);
            ag_p = __builtin_amdgcn_readfirstlane(l.y);
            ag_y = *reinterpret_cast<const float2 *>(yrow);
            return;
        }
        const int r = m - 1;
        const float2 y = ag_y;
        if (r < 7) ag_y = *reinterpret_cast<const float2 *>(yrow + (size_t)(r + 1) * ER_GSTRIDE);
        if (r < ag_nv) {
            ag_acc.x += y.x; ag_acc.y += y.y;
            if (r == ag_nv - 1 || ag_d[(r + 1) & 7] != ag_d[r]) {
                typedef int i32x2 __attribute__((ext_vector_type(2)));
                i32x2 v; v[0] = __float_as_int(ag_acc.x); v[1] = __float_as_int(ag_acc.y);
                __builtin_amdgcn_raw_buffer_store_b64(v, r_pc, ag_p * 512 + lane * 8, 0, 0);
                ag_p++;
                ag_acc = make_float2(0.f, 0.f);
            }
        }
    };
    // ---- loaders.  A wave brings in rows 8w .. 8w + 7 of a tile, two rows per instruction (half-wave per row, 16 bytes per lane): global
    // memory only ever sees whole rows.  Buffer loads: what lies past the last row reads as zero (edge rows) / index 0 (gathers)
    const __amdgpu_buffer_rsrc_t r_e0 = __builtin_amdgcn_make_buffer_rsrc((void *)e0, 0, NARROW ? (int)(M * in_cols * 4) : (int)(M * 512), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_ia = __builtin_amdgcn_make_buffer_rsrc((void *)ia, 0, (int)(M * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_ib = __builtin_amdgcn_make_buffer_rsrc((void *)ib, 0, (int)(M * 8), 0x00020000);
    const int ix_lane = (8 * w + h) * 8;
    // the gather indices of the wave's rows, already where the gathers want them: lane (n, h), k <-> row 8w + 2k + h (8 operations; one
    // 8-lane load per array + a lane exchange measured 2 % slower, tools/edge_mlp3_lib_ab.sh)
    auto idx_op = [&](int m, unsigned tile_rows, int (&ja)[4], int (&jb)[4]) __attribute__((always_inline)) {
        const int k = m >> 1;
        if (NARROW || (EM_SKIP & 512)) return;
        if (m & 1) jb[k] = __builtin_amdgcn_raw_buffer_load_b32(r_ib, ix_lane + tile_rows * 8 + 16 * k, 0, 0);
        else ja[k] = __builtin_amdgcn_raw_buffer_load_b32(r_ia, ix_lane + tile_rows * 8 + 16 * k, 0, 0);
    };
    auto g_issue_op = [&](int m, float4 (&GA)[4], float4 (&GB)[4], const int (&ja)[4], const int (&jb)[4]) __attribute__((always_inline)) {      // 8 operations
        const int k = m >> 1;
        if (NARROW || (EM_SKIP & 256)) return;
        if (m & 1) GB[k] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(xb) + (size_t)((unsigned)jb[k] * 512u + 16u * n));
        else GA[k] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(xa) + (size_t)((unsigned)ja[k] * 512u + 16u * n));
    };
    // G = (xa[dst] + xb[src] + b0) / alpha, what layer 1's accumulators start from: 12 operations
    auto g_commit_op = [&](int m, float4 (&GA)[4], float4 (&GB)[4], float *Gt) __attribute__((always_inline)) {
        const int k = m / 3, part = m % 3;
        if (NARROW) {      // (no gathers: layer 1 starts from its bias)
            if (part == 2) *reinterpret_cast<float4 *>(Gt + (size_t)(8 * w + 2 * k + h) * ER_GSTRIDE + 4 * n) = b0v;
            return;
        }
        if (part == 0) { GA[k].x += GB[k].x; GA[k].y += GB[k].y; GA[k].z += GB[k].z; GA[k].w += GB[k].w; }
        else if (part == 1) {
            GA[k].x = fmaf(GA[k].x, inv_alpha, b0v.x); GA[k].y = fmaf(GA[k].y, inv_alpha, b0v.y);
            GA[k].z = fmaf(GA[k].z, inv_alpha, b0v.z); GA[k].w = fmaf(GA[k].w, inv_alpha, b0v.w);
        } else *reinterpret_cast<float4 *>(Gt + (size_t)(8 * w + 2 * k + h) * ER_GSTRIDE + 4 * n) = GA[k];
    };
    auto e_issue_op = [&](int k, float4 (&E)[4], unsigned tile_off) __attribute__((always_inline)) {      // 4 operations
        if (NARROW) {
            // (MODE 2) the rows are [M][in_cols] floats, in_cols a multiple of 4 up to 128: the lanes that stand for columns past in_cols hold
            // zeros (layer 1's packed weight is zero there too), a row's real columns are one or a few 16-byte reads
            const unsigned rowb = ((tile_off >> 9) + 8 * w + 2 * k + h) * (unsigned)(in_cols * 4);
            const float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_e0, rowb + 16 * n, 0, 0));
            E[k] = 4 * n < in_cols ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
        if (!(EM_SKIP & 128)) E[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_e0, ld_lane + tile_off + 1024 * k, 0, 0));
    };
    // an edge row's 16 bytes (times cs) cut into the NP pieces, parked as layer 1's B operand: per 16 bytes (scale) (pack, write), then per
    // further piece 4 x (-) and (pack, write)
    constexpr int EC_ROW = 2 + 5 * (NP - 1), EC_OPS = 4 * EC_ROW;
    unsigned eq0 = 0, eq1 = 0;
    auto e_commit_op = [&](int m, float4 (&E)[4], el16 *Xtile) __attribute__((always_inline)) {
        const int k = m / EC_ROW, o = m % EC_ROW;
        el16 *dst = Xtile + (size_t)(8 * w + 2 * k + h) * EM_STRIDE + 4 * n;
        if (o == 0) {
            if (F16) { E[k].x *= cs; E[k].y *= cs; E[k].z *= cs; E[k].w *= cs; }
            return;
        }
        const int oo = o - 1;
        if (oo % 5 == 0) {
            const int p = oo / 5;
            eq0 = pk(E[k].x, E[k].y); eq1 = pk(E[k].z, E[k].w);
            if (p < NP - 1) { opaque(eq0); opaque(eq1); }
            *reinterpret_cast<uint2 *>(dst + (size_t)p * ER_TILE_P) = make_uint2(eq0, eq1);
        }
        else if (oo % 5 == 1) E[k].x -= lo_f(eq0);
        else if (oo % 5 == 2) E[k].y -= hi_f(eq0);
        else if (oo % 5 == 3) E[k].z -= lo_f(eq1);
        else E[k].w -= hi_f(eq1);
    };

    // =================== a phase: one layer of one tile, NS MFMAs on one accumulation chain, with side(k) riding behind MFMA k.
    // acc starts from 16 floats of an LDS row (register r <-> feature 32w + 8(r >> 2) + 4h + (r & 3)); the step's NP B operands are
    // read one step ahead, the piece the next step needs first first.  (weight piece, activation piece) of a step's products, small
    // terms first -- bf16: the six that matter of nine; fp16: three of four
    // the accumulators' start (G row of the tile for layer 1, the bias table for layers 2 and 3): 4 LDS reads.  What they read does not
    // depend on the phase's barrier, so the phase BEFORE requests them in its last gaps, once the accumulator's previous content has been
    // consumed: the first MFMA behind a barrier then waits for its B operand only
    auto start_op = [&](const float *init, f32x16 &acc) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 t = *reinterpret_cast<const float4 *>(init + 32 * w + 8 * q + 4 * h);
            acc[4 * q] = t.x; acc[4 * q + 1] = t.y; acc[4 * q + 2] = t.z; acc[4 * q + 3] = t.w;
        }
    };
    auto phase = [&](int l, const el16 *Xtile, const float *init, f32x16 &acc, auto &&side) __attribute__((always_inline)) {
        constexpr int NPROD = C::NPROD;
        constexpr int WP[6] = {0, F16 ? 1 : 2, F16 ? 0 : 1, 0, 1, 0}, XP[6] = {F16 ? 1 : 2, 0, F16 ? 0 : 1, 1, 0, 0};
        constexpr int RD[6] = {F16 ? 1 : -1, F16 ? 0 : 2, -1, 0, -1, 1};      // the next step's piece requested behind MFMA i
        const el16 *row = Xtile + (size_t)n * EM_STRIDE + 64 * h;
        i32x4 bc[NP], bn[NP];
        bc[XP[0]] = *reinterpret_cast<const i32x4 *>(row + XP[0] * ER_TILE_P);
        if (init) start_op(init, acc);      // (else: requested by the previous phase's last gaps -- nothing of it waits for this phase's barrier)
#pragma unroll
        for (int p = 0; p < NP; p++)
            if (p != XP[0]) bc[p] = *reinterpret_cast<const i32x4 *>(row + p * ER_TILE_P);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int st = 0; st < 8; st++) {
#pragma unroll
            for (int i = 0; i < NPROD; i++) {
                mfma((l * NP + WP[i]) * 8 + st, bc[XP[i]], acc);
                if (RD[i] >= 0 && st < 7) bn[RD[i]] = *reinterpret_cast<const i32x4 *>(row + RD[i] * ER_TILE_P + 8 * (st + 1));
#ifndef EM_NOSIDE      // (timing experiment: the bare MFMA pipeline -- results wrong)
                side(NPROD * st + i);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int p = 0; p < NP; p++) bc[p] = bn[p];
        }
    };

    // Which tiles a workgroup takes.  Workgroup b runs on XCD b % 8, and every XCD has its own L2: with the tiles dealt round-robin each L2
    // would have to hold the gathered node rows of the WHOLE graph (10 MB at N = 1e4 against 4 MB: ~55 MB of the launch's 209 MB of
    // reads were gathers missing it).  So the tile sequence is cut into 8 contiguous eighths, one per XCD, and each eighth into contiguous
    // ranges of pairs, one per workgroup of that XCD: edges are in destination order, so an XCD's workgroups gather from one region of
    // the node tables.  (Grids that are not a multiple of 8: plain contiguous ranges.)
    const int ntiles = (int)((M + 31) / 32), npairs = (ntiles + 1) / 2, G = (int)gridDim.x;
    const int wg = (G % 8 == 0) ? (int)(blockIdx.x & 7) * (G / 8) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int T0 = 2 * (int)((int64_t)wg * npairs / G), Tend = 2 * (int)((int64_t)(wg + 1) * npairs / G), stride = 1;
    constexpr int XT = C::XT;
    el16 *const XA = sX, *const XB = sX + 2 * XT;       // slot s, buffer b: sX + (2s + b) * XT
    float *const GtA = sG, *const GtB = sG + 32 * ER_GSTRIDE, *const YtA = sY, *const YtB = sY + 32 * ER_GSTRIDE;
    float2 *const SrA = sS + (size_t)n * 4, *const SrB = sS + (size_t)(32 + n) * 4;
    // Memory schedule of a pair cycle.  By elimination (tools/edge_mlp3_skip_ab.sh, fp16 pieces, 115 us: without the rows out 91, without the
    // edge rows 96, without the gathers 101, without the index loads 108, without the ReLU + cut's ~290 vector instructions 113, bare MFMA
    // pipeline 68) the kernel spends what it spends beyond its MFMAs on MEMORY instructions -- one L1 / address unit per CU, four waves in
    // step -- not on the ~1,400 vector instructions per pair that ride in the gaps.  Requesting a tile's 12 loads together at the top of a
    // phase, a phase earlier (so that no wait stands behind the rows out: vmcnt counts stores too, in order), measured 5 % SLOWER: what
    // is below spreads the requests over the phases.
    int jaA[4], jbA[4], jaB[4], jbB[4];
    float4 EA[4], EB[4], GAa[4], GBa[4], GAb[4], GBb[4];
    {   // the first two tiles' inputs, synchronously
#pragma unroll
        for (int m = 0; m < 8; m++) { idx_op(m, (unsigned)T0 * 32u, jaA, jbA); idx_op(m, (unsigned)(T0 + stride) * 32u, jaB, jbB); }
#pragma unroll
        for (int m = 0; m < 8; m++) g_issue_op(m, GAa, GBa, jaA, jbA);
#pragma unroll
        for (int k = 0; k < 4; k++) { e_issue_op(k, EA, (unsigned)T0 * 16384u); e_issue_op(k, EB, (unsigned)(T0 + stride) * 16384u); }
#pragma unroll
        for (int m = 0; m < 12; m++) g_commit_op(m, GAa, GBa, GtA);
#pragma unroll
        for (int m = 0; m < 8; m++) g_issue_op(m, GAb, GBb, jaB, jbB);
#pragma unroll
        for (int m = 0; m < EC_OPS; m++) e_commit_op(m, EA, XA);      // (one list at a time: the operations of a list share their temporaries)
#pragma unroll
        for (int m = 0; m < EC_OPS; m++) e_commit_op(m, EB, XB);
#pragma unroll
        for (int m = 0; m < 12; m++) g_commit_op(m, GAb, GBb, GtB);
    }
    f32x16 accA, accB, accLA, accLB;
#pragma unroll
    for (int r = 0; r < 16; r++) accLA[r] = accLB[r] = 0.f;
    unsigned offA_prev = 0xfff00000u, offB_prev = 0xfff00000u;       // (no rows to write yet: past the end of any buffer this kernel takes)
    int tA_prev = 0x3fffffff, tB_prev = 0x3fffffff;                  // (AGG: a tile past the last row has no rows to sum)
    __syncthreads();
    start_op(GtA + (size_t)n * ER_GSTRIDE, accA);
#define SL(a) ((a) * NS / 48)      /* gap ranges below are written for 48 gaps per phase */
    int x = 0;
    for (int tA = T0; tA < Tend; tA += 2 * stride, x ^= 1) {
        const int tB = tA + stride, tA2 = tA + 2 * stride, tB2 = tB + 2 * stride;
        el16 *const XA0 = XA + x * XT, *const XA1 = XA + (x ^ 1) * XT, *const XB0 = XB + x * XT, *const XB1 = XB + (x ^ 1) * XT;
        stamp();
        // 0: layer 1 of A | LayerNorm partials of the previous B, LayerNorm's end + rows out of the previous A, the next A's indices
        phase(0, XA0, nullptr, accA, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(GtB + (size_t)n * ER_GSTRIDE, accB));
            if (!(EM_SKIP & 2)) ER_SPREAD(k, SL(0), SL(18), LNP_OPS, lnp_op(m, accLB, SrB));
            if (!(EM_SKIP & 4)) ER_SPREAD(k, SL(14), SL(44), LNF_OPS, lnf_op(m, accLA, SrA, offA_prev, YtA));
            if (!(EM_SKIP & 32)) ER_SPREAD(k, SL(40), SL(48), 8, idx_op(m, (unsigned)tA2 * 32u, jaA, jbA));
            if (AGG) ER_SPREAD(k, SL(44), SL(46), 1, agg_load_op(tA_prev, ag_lA));
        });
        __syncthreads();
        stamp();
        // 1: layer 1 of B | A's ReLU + pieces, LayerNorm's end + rows out of the previous B, the next B's indices
        phase(0, XB0, nullptr, accB, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(sT, accA));
            if (!(EM_SKIP & 4)) ER_SPREAD(k, SL(0), SL(32), LNF_OPS, lnf_op(m, accLB, SrB, offB_prev, YtB));
            if (AGG) ER_SPREAD(k, SL(6), SL(42), 9, agg_op(m, YtA, tA_prev, ag_lA));
            if (AGG) ER_SPREAD(k, SL(44), SL(46), 1, agg_load_op(tB_prev, ag_lB));
            else if (C::ROWS_VIA_LDS && !(EM_SKIP & 4)) ER_SPREAD(k, SL(8), SL(40), 8, rows_out_op(m, YtA, offA_prev));
            if (!(EM_SKIP & 1)) ER_SPREAD(k, SL(0), SL(44), RELU_OPS, relu_op(m, accA, XA1));
            if (!(EM_SKIP & 32)) ER_SPREAD(k, SL(40), SL(48), 8, idx_op(m, (unsigned)tB2 * 32u, jaB, jbB));
            if (!(EM_SKIP & 8)) ER_SPREAD(k, SL(32), SL(48), 8, g_issue_op(m, GAa, GBa, jaA, jbA));
        });
        __syncthreads();
        stamp();
        // 2: layer 2 of A | B's ReLU + pieces, the next A's gathers
        phase(1, XA1, nullptr, accA, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(sT, accB));
            if (!(EM_SKIP & 8)) ER_SPREAD(k, SL(32), SL(48), 8, g_issue_op(m, GAb, GBb, jaB, jbB));
            if (!(EM_SKIP & 16)) ER_SPREAD(k, SL(32), SL(40), 4, e_issue_op(m, EA, (unsigned)tA2 * 16384u));
            if (AGG) ER_SPREAD(k, SL(8), SL(44), 9, agg_op(m, YtB, tB_prev, ag_lB));
            else if (C::ROWS_VIA_LDS && !(EM_SKIP & 4)) ER_SPREAD(k, SL(8), SL(32), 8, rows_out_op(m, YtB, offB_prev));
            if (!(EM_SKIP & 1)) ER_SPREAD(k, SL(0), SL(44), RELU_OPS, relu_op(m, accB, XB1));
            if (!(EM_SKIP & 8)) ER_SPREAD(k, SL(20), SL(44), 12, g_commit_op(m, GAa, GBa, GtA));
        });
        __syncthreads();
        stamp();
        // 3: layer 2 of B | A's ReLU + pieces, the next B's gathers, the next A's edge rows requested
        phase(1, XB1, nullptr, accB, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(sT + EM_N, accLA));
            if (!(EM_SKIP & 16)) ER_SPREAD(k, SL(32), SL(40), 4, e_issue_op(m, EB, (unsigned)tB2 * 16384u));
            if (!(EM_SKIP & 1)) ER_SPREAD(k, SL(0), SL(48), RELU_OPS, relu_op(m, accA, XA0));
            if (!(EM_SKIP & 8)) ER_SPREAD(k, SL(20), SL(44), 12, g_commit_op(m, GAb, GBb, GtB));
        });
        __syncthreads();
        stamp();
        // 4: layer 3 of A | B's ReLU + pieces, the next A's edge rows cut and parked, the next B's requested
        phase(2, XA0, nullptr, accLA, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(sT + EM_N, accLB));
            if (!(EM_SKIP & 1)) ER_SPREAD(k, SL(0), SL(48), RELU_OPS, relu_op(m, accB, XB0));
            if (!(EM_SKIP & 16)) ER_SPREAD(k, SL(4), SL(48), EC_OPS, e_commit_op(m, EA, XA1));
        });
        __syncthreads();
        stamp();
        // 5: layer 3 of B | A's LayerNorm partials, the next B's edge rows cut and parked
        phase(2, XB0, nullptr, accLB, [&](int k) __attribute__((always_inline)) {
            ER_SPREAD(k, SL(46), SL(48), 1, start_op(GtA + (size_t)n * ER_GSTRIDE, accA));
            if (!(EM_SKIP & 2)) ER_SPREAD(k, SL(0), SL(20), LNP_OPS, lnp_op(m, accLA, SrA));
            if (!(EM_SKIP & 16)) ER_SPREAD(k, SL(4), SL(48), EC_OPS, e_commit_op(m, EB, XB1));
        });
        offA_prev = (unsigned)tA * 16384u; offB_prev = (unsigned)tB * 16384u;
        tA_prev = tA; tB_prev = tB;
        __syncthreads();
    }
    // the pipeline's tail: the last B's partials, both tiles' LayerNorm ends, their rows out
#pragma unroll
    for (int m = 0; m < LNP_OPS; m++) lnp_op(m, accLB, SrB);
#pragma unroll
    for (int m = 0; m < LNF_OPS; m++) lnf_op(m, accLA, SrA, offA_prev, YtA);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < LNF_OPS; m++) lnf_op(m, accLB, SrB, offB_prev, YtB);
    if (AGG) {
        agg_load_op(tA_prev, ag_lA);
        agg_load_op(tB_prev, ag_lB);
#pragma unroll
        for (int m = 0; m < 9; m++) agg_op(m, YtA, tA_prev, ag_lA);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 9; m++) agg_op(m, YtB, tB_prev, ag_lB);
    } else if (C::ROWS_VIA_LDS) {
#pragma unroll
        for (int m = 0; m < 8; m++) rows_out_op(m, YtA, offA_prev);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; m++) rows_out_op(m, YtB, offB_prev);
    }
#undef SL
}

// =====================================================================================================================================
// k_node_update_b3 -- the node update of an InteractionNetwork layer (+ the next layer's node-level products) on the same machinery:
//   h = relu(agg Wa^T + x Wx^T + b0);  h = relu(h W2^T + b2);  x' = LayerNorm(h W3^T + b3) + x;  xa' = x' Wi^T;  xb' = x' Wj^T
// (/root/reference/meshnet/graph_network.py:203-222).  Rounds 2-5 ran it on the exact-fp32 MFMA with the weights transposed through LDS
// by scalar writes (k_node_update, csplat_gemm.hip: 44 us at N = 1e4, 0.66 of the 3.0 ms rollout step).  Here: 16-bit pieces as in the edge
// kernel (Piece<F16>: two fp16 pieces, three products, a fixed 2^-4 scale; else three bf16 pieces, six products), weights PRE-PACKED as MFMA A
// operands (csplat_gnn_node_update_pack: [matrix 6][wave 4][piece 3][step 8][lane] x 16 bytes) and streamed from L2 into registers half
// a product ahead; one 32-row tile per 4-wave workgroup, wave j = output features 32j .. 32j + 31, activations between the layers as
// piece tiles in LDS (PieceChain<F16> below, which k_rows_chain runs on as well).  ~160 registers and 80 KB of LDS: two workgroups per CU,
// which is what fills the gaps (the layers of a tile are a dependent chain).  (Two tiles per workgroup sharing each weight operand -- half the 576 KB of packed weights per row through the L1 --
// measured SLOWER, 36.9 against 30.3 us: the chain of six products per tile, not the weight traffic, is what a workgroup waits for.)
constexpr int NB_MATS = 6;                                         // Wa, Wx, W2, W3, Wi', Wj'
constexpr size_t NB_IMAGE_BYTES = (size_t)NB_MATS * 4 * 3 * 8 * 64 * 16;      // 589,824
constexpr int NB_XT = 3 * ER_TILE_P;
constexpr size_t NB_LDS_BYTES = (size_t)3 * NB_XT * 2 + 32 * 4 * 8;           // three piece tiles + LayerNorm partials

template <bool F16>
__global__ __launch_bounds__(64) void k_node_pack(const float *__restrict__ W0, const float *__restrict__ W1, const float *__restrict__ W2,
                                                  const float *__restrict__ W3, const float *__restrict__ W4, const float *__restrict__ W5,
                                                  i32x4 *__restrict__ img) {
    // block = (matrix, wave j, step st); lane (m, h): the 8 contraction elements of output feature 32j + m it feeds into step st.
    // Matrices 0, 1 contract over rows as they lie in memory; 2 .. 5 over what the previous layer's waves left in LDS (er_src_col)
    const int st = blockIdx.x & 7, j = (blockIdx.x >> 3) & 3, mat = blockIdx.x >> 5;
    const float *W = mat == 0 ? W0 : mat == 1 ? W1 : mat == 2 ? W2 : mat == 3 ? W3 : mat == 4 ? W4 : W5;
    if (!W) return;
    const int lane = threadIdx.x, m = lane & 31, h = lane >> 5;
    constexpr int NP = Piece<F16>::NP;
    i32x4 op[3];
    pack_operands<F16>(W, (size_t)(32 * j + m) * EM_N, mat < 2 ? 0 : 1, h, st, op);
#pragma unroll
    for (int q = 0; q < NP; q++) img[((size_t)((mat * 4 + j) * NP + q) * 8 + st) * 64 + lane] = op[q];
}

// PieceChain -- what a wave of k_node_update_b3 and k_rows_chain (below) works with: one 32-row tile per 4-wave workgroup, a chain of
// 128-wide products on it.  Lane (n, h) of wave w holds, in an accumulator, features 32w + 8(r >> 2) + 4h + (r & 3) of row n.
// F16: two fp16 pieces per operand, three products per step -- half the MFMAs of the layers' dependent chain.  fp16's range is kept by
// running everything multiplied by SC = 2^-4 (exact: ReLU is homogeneous, LayerNorm takes SC^2 eps, the next layer's products are
// multiplied back): aggregates and latents up to ~1e6 in magnitude fit, and an element below 2 of the original units keeps an absolute
// error of 5e-7 -- node latents and aggregates of LayerNorm'd messages are O(1 .. 100).
template <bool F16> struct PieceChain {
    typedef Piece<F16> P;
    static constexpr int NP = P::NP, NPROD = P::NPROD;
    static constexpr float SC = P::SC;
    const int lane, w, n, h;
    const int64_t N, row0, grow;      // (grow: the row this lane holds in an accumulator)
    const i32x4 *const img;
    i32x4 wq[2][4 * NP];      // weights: the 24 A operands of a product in two halves (steps 0-3, 4-7), each requested half a product ahead

    __device__ __forceinline__ PieceChain(int64_t N_, const i32x4 *__restrict__ img_)
        : lane(threadIdx.x & 63), w(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), n(lane & 31), h(lane >> 5), N(N_),
          row0((int64_t)blockIdx.x * 32), grow(row0 + n), img(img_) {
        fetch(0, 0);
        fetch(0, 1);
    }
    __device__ __forceinline__ void fetch(int mat, int half) {
        const i32x4 *src = img + ((size_t)(mat * 4 + w) * NP * 8) * 64 + lane;
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++) wq[half][p * 4 + s4] = src[(size_t)(p * 8 + 4 * half + s4) * 64];
    }
    // the tile's rows of src, whole rows per instruction (half-wave per row), cut into pieces -> tile Bt
    __device__ __forceinline__ void cut_rows(const float *__restrict__ src, el16 *Bt, const int *__restrict__ piece_ptr = nullptr) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int64_t row = row0 + 8 * w + 2 * k + h;
            row = row < N ? row : N - 1;
            if (piece_ptr) {
                // the rows arrive as the edge launch's "pieces" (csplat_gnn_edge_mlp3): node `row` owns pieces piece_ptr[row] ..
                // piece_ptr[row + 1] - 1, summed here in that order -- what csplat_gnn_segment_sum over the pieces would have written
                const int p0 = piece_ptr[row], p1 = piece_ptr[row + 1];
                float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int p = p0; p < p1; p++) {
                    const float4 t = *reinterpret_cast<const float4 *>(src + (size_t)p * EM_N + 4 * n);
                    acc4.x += t.x; acc4.y += t.y; acc4.z += t.z; acc4.w += t.w;
                }
                v[k] = acc4;
            } else v[k] = *reinterpret_cast<const float4 *>(src + row * EM_N + 4 * n);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            el16 *dst = Bt + (size_t)(8 * w + 2 * k + h) * EM_STRIDE + 4 * n;
            float e[4] = {v[k].x * SC, v[k].y * SC, v[k].z * SC, v[k].w * SC};
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const unsigned q0 = P::pk(e[0], e[1]), q1 = P::pk(e[2], e[3]);
                *reinterpret_cast<uint2 *>(dst + (size_t)p * ER_TILE_P) = make_uint2(q0, q1);
                e[0] -= P::lo_f(q0); e[1] -= P::hi_f(q0); e[2] -= P::lo_f(q1); e[3] -= P::hi_f(q1);
            }
        }
    }
    // one product: acc += W_mat (registers) x tile (pieces in LDS); the next weights are requested as the halves free up
    __device__ __forceinline__ void product(const el16 *Bt, f32x16 &acc, int next_mat) {
        constexpr int WP[6] = {0, F16 ? 1 : 2, F16 ? 0 : 1, 0, 1, 0}, XP[6] = {F16 ? 1 : 2, 0, F16 ? 0 : 1, 1, 0, 0};
        const el16 *row = Bt + (size_t)n * EM_STRIDE + 64 * h;
        i32x4 bc[NP], bn[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) bc[p] = *reinterpret_cast<const i32x4 *>(row + p * ER_TILE_P);
#pragma unroll
        for (int st = 0; st < 8; st++) {
            if (st < 7) {
#pragma unroll
                for (int p = 0; p < NP; p++) bn[p] = *reinterpret_cast<const i32x4 *>(row + p * ER_TILE_P + 8 * (st + 1));
            }
#pragma unroll
            for (int i = 0; i < NPROD; i++) {
                if (F16) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, wq[st >> 2][WP[i] * 4 + (st & 3)]),
                                                                      __builtin_bit_cast(f16x8v, bc[XP[i]]), acc, 0, 0, 0);
                else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8v, wq[st >> 2][WP[i] * 4 + (st & 3)]),
                                                                   __builtin_bit_cast(bf16x8v, bc[XP[i]]), acc, 0, 0, 0);
            }
            if (st == 3 && next_mat >= 0) fetch(next_mat, 0);
#pragma unroll
            for (int p = 0; p < NP; p++) bc[p] = bn[p];
        }
        if (next_mat >= 0) fetch(next_mat, 1);
    }
    __device__ __forceinline__ void start_from(const float *__restrict__ b, f32x16 &acc) const {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 t = b ? *reinterpret_cast<const float4 *>(b + 32 * w + 8 * q + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc[4 * q] = t.x * SC; acc[4 * q + 1] = t.y * SC; acc[4 * q + 2] = t.z * SC; acc[4 * q + 3] = t.w * SC;
        }
    }
    // 16 values of row n -> the next product's pieces, positions 32w + 16h .. + 15
    __device__ __forceinline__ void to_pieces(const float (&v)[16], el16 *Bt, float scale) const {
        float e[16];
#pragma unroll
        for (int r = 0; r < 16; r++) e[r] = F16 ? v[r] * scale : v[r];
        el16 *dst = Bt + (size_t)n * EM_STRIDE + 32 * w + 16 * h;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            unsigned q[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { q[j] = P::pk(e[2 * j], e[2 * j + 1]); e[2 * j] -= P::lo_f(q[j]); e[2 * j + 1] -= P::hi_f(q[j]); }
            *reinterpret_cast<uint4 *>(dst + (size_t)p * ER_TILE_P) = make_uint4(q[0], q[1], q[2], q[3]);
            *reinterpret_cast<uint4 *>(dst + (size_t)p * ER_TILE_P + 8) = make_uint4(q[4], q[5], q[6], q[7]);
        }
    }
    __device__ __forceinline__ void store_rows(const float (&v)[16], float *__restrict__ dst) const {
        if (grow < N) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                *reinterpret_cast<float4 *>(dst + grow * EM_N + 32 * w + 8 * q + 4 * h) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    }
    // a bare product dst = tile W^T in the original units, from the weights in the registers
    __device__ __forceinline__ void plain_product(const el16 *Bt, int next_mat, float *__restrict__ dst) {
        f32x16 acc;
        float v[16];
        start_from(nullptr, acc);
        product(Bt, acc, next_mat);
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = acc[r] * P::ISC;
        store_rows(v, dst);
    }
};

template <bool F16>
__global__ __launch_bounds__(256, 2) void k_node_update_b3(int64_t N, const float *__restrict__ agg, const float *__restrict__ x,
                                                           const i32x4 *__restrict__ img, const float *__restrict__ b0,
                                                           const float *__restrict__ b2, const float *__restrict__ b3,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                           int has_next, float *__restrict__ x_new, float *__restrict__ xa,
                                                           float *__restrict__ xb, const int *__restrict__ piece_ptr) {
    extern __shared__ char s_mem[];
    el16 *const B0 = reinterpret_cast<el16 *>(s_mem), *const B1 = B0 + NB_XT, *const B2 = B0 + 2 * NB_XT;      // three tiles of three pieces
    float2 *const sS = reinterpret_cast<float2 *>(s_mem + (size_t)3 * NB_XT * 2);             // [32][wave 4] (sum, M2)
    constexpr float SC = Piece<F16>::SC;
    eps *= SC * SC;
    PieceChain<F16> c(N, img);
    const int w = c.w, n = c.n, h = c.h;
    c.cut_rows(agg, B0, piece_ptr);
    c.cut_rows(x, B1);
    // the residual's x in the accumulators' layout (register r <-> feature 32w + 8(r >> 2) + 4h + (r & 3) of row n)
    float4 xres[4];
    {
        int64_t row = c.row0 + n;
        row = row < N ? row : N - 1;
#pragma unroll
        for (int q = 0; q < 4; q++) xres[q] = *reinterpret_cast<const float4 *>(x + row * EM_N + 32 * w + 8 * q + 4 * h);
    }
    __syncthreads();
    f32x16 acc;
    float v[16];
    // ---- layer 1 (K = 256: agg and x)
    c.start_from(b0, acc);
    c.product(B0, acc, 1);
    c.product(B1, acc, 2);
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = relu_keep_nan(acc[r]);
    c.to_pieces(v, B2, 1.f);
    __syncthreads();
    // ---- layer 2
    c.start_from(b2, acc);
    c.product(B2, acc, 3);
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = relu_keep_nan(acc[r]);
    c.to_pieces(v, B0, 1.f);
    __syncthreads();
    // ---- layer 3, LayerNorm (the four waves' partials combined by the parallel-variance formula), residual
    c.start_from(b3, acc);
    c.product(B0, acc, has_next ? 4 : -1);
    {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) s += acc[r];
        s = pair_sum(s);
        const float mj = s * (1.f / 32.f);
        float m2 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) { const float d = acc[r] - mj; m2 = fmaf(d, d, m2); }
        m2 = pair_sum(m2);
        sS[n * 4 + w] = make_float2(s, m2);
    }
    __syncthreads();
    {
        const float4 u0 = *reinterpret_cast<const float4 *>(sS + n * 4), u1 = *reinterpret_cast<const float4 *>(sS + n * 4 + 2);
        const float mean = ((u0.x + u0.z) + (u1.x + u1.z)) * (1.f / EM_N);
        const float d0 = u0.x * (1.f / 32.f) - mean, d1 = u0.z * (1.f / 32.f) - mean, d2 = u1.x * (1.f / 32.f) - mean, d3 = u1.z * (1.f / 32.f) - mean;
        const float m2 = ((u0.y + u0.w) + (u1.y + u1.w)) + 32.f * ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
        const float rstd = rsqrtf(m2 * (1.f / EM_N) + eps);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int f = 32 * w + 8 * q + 4 * h;
            const float4 ga = *reinterpret_cast<const float4 *>(gamma + f), be = *reinterpret_cast<const float4 *>(beta + f);
            v[4 * q] = (acc[4 * q] - mean) * rstd * ga.x + be.x + xres[q].x; v[4 * q + 1] = (acc[4 * q + 1] - mean) * rstd * ga.y + be.y + xres[q].y;
            v[4 * q + 2] = (acc[4 * q + 2] - mean) * rstd * ga.z + be.z + xres[q].z; v[4 * q + 3] = (acc[4 * q + 3] - mean) * rstd * ga.w + be.w + xres[q].w;
        }
    }
    c.store_rows(v, x_new);
    if (!has_next) return;
    // ---- the next layer's node-level products of the updated latents
    c.to_pieces(v, B1, SC);
    __syncthreads();
    c.plain_product(B1, 5, xa);
    c.plain_product(B1, -1, xb);
}

// A CHAIN of 128-wide Linears on node rows, PieceChain<F16> again (pre-packed 16-bit-piece weights streamed into registers half a
// product ahead, one 32-row tile per workgroup), round 6 -- what the rollout step still ran as four launches of the exact-fp32
// k_linear128_rows32 (16 us each at N = 10^4: latency-sized):
//   MODE 0: out_a = x Wa^T, out_b = x Wb^T                 (the first processor layer's x_i / x_j products, graph_network.py:178-199)
//   MODE 1: out_a = relu(W1 relu(W0 x + b0) + b1)          (the decoder's two hidden layers, graph_network.py:295-332)
// image = csplat_gnn_rows_chain_pack: matrix slots 0 / 1 (MODE 0: Wa, Wb -- both contract over the rows as they lie in memory) or
// 0 / 2 (MODE 1: W0 over the rows, W1 over what the first layer's waves left in LDS).
template <bool F16, int MODE>
__global__ __launch_bounds__(256, 2) void k_rows_chain(int64_t N, const float *__restrict__ x, const i32x4 *__restrict__ img,
                                                       const float *__restrict__ b0, const float *__restrict__ b1,
                                                       float *__restrict__ out_a, float *__restrict__ out_b) {
    extern __shared__ char s_mem[];
    el16 *const B0 = reinterpret_cast<el16 *>(s_mem), *const B1 = B0 + NB_XT;                 // tiles of three pieces (the node update's layout)
    constexpr float ISC = Piece<F16>::ISC;
    PieceChain<F16> c(N, img);
    c.cut_rows(x, B0);
    __syncthreads();
    f32x16 acc;
    float v[16];
    if (MODE == 0) {
        c.plain_product(B0, 1, out_a);
        c.plain_product(B0, -1, out_b);
    } else {
        c.start_from(b0, acc);
        c.product(B0, acc, 2);
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = relu_keep_nan(acc[r]);
        c.to_pieces(v, B1, 1.f);
        __syncthreads();
        c.start_from(b1, acc);
        c.product(B1, acc, -1);
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = relu_keep_nan(acc[r]) * ISC;
        c.store_rows(v, out_a);
    }
}

}  // namespace

// 0: two fp16 pieces (default), 1: three bf16 pieces (header).  The image is laid out for the mode it is packed under; callers re-pack when
// they change the mode (meshnet/graph_network.py keys its cache on it)
static int g_em_mode = 0;
extern "C" int csplat_gnn_edge_mlp3_mode(int mode) {
    const int was = g_em_mode;
    if (mode == 0 || mode == 1) g_em_mode = mode;
    return was;
}

// ---- what the entry points below share
template <int I> using int_c = std::integral_constant<int, I>;
// the one mode dispatch: f(std::bool_constant<F16>) under the current piece mode, so that a launch's argument list is written once
template <class F> static int by_mode(F &&f) { return g_em_mode == 0 ? f(std::true_type{}) : f(std::false_type{}); }
// `bytes` of dynamic LDS for KERNEL: the runtime is asked once per kernel, a refusal is the caller's error `what`
template <auto KERNEL> static int need_lds(size_t bytes, const char *what) {
    static const bool ok = [bytes] {
        const bool granted = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
        (void)hipGetLastError();
        return granted;
    }();
    CSPLAT_REQUIRE(ok, what);
    return 0;
}
template <class... T> static bool aligned16(const T *...p) { return ((... | (uintptr_t)p) & 15u) == 0; }

// k_edge_mlp3r<F16, MODE> over M rows of in_cols floats, for csplat_gnn_edge_mlp3 and csplat_gnn_mlp3_rows.  The kernel addresses its rows
// through 32-bit buffer offsets (rows past the end dropped by the hardware's bounds check): 2^22 rows = 2 GiB of [.,128] floats per launch,
// longer inputs go out in chunks.  This owns the chunk size, the grid rule and the per-chunk offsets of every per-row operand.
// CSPLAT_EM_CHUNK_ROWS (a test-only hook: a smaller chunk, a multiple of 64, so that tests reach the loop) holds for BOTH entries since the
// two loops became this one; csplat_gnn_mlp3_rows did not read it before.
template <bool F16, int MODE>
static int em_launch_chunks(hipStream_t s, const char *lds_refused, int64_t M, const float *e0, int in_cols, float alpha, const float *e0_absmax,
                            const float *xa, const int64_t *ia, const float *xb, const int64_t *ib, const void *image, const float *b0,
                            const float *b1, const float *b2, const float *gamma, const float *beta, float eps, float *out,
                            const int32_t *group_piece0, float *pieces) {
    if (const int e = need_lds<k_edge_mlp3r<F16, MODE>>(ErCfg<F16>::LDS_BYTES, lds_refused)) return e;
    ProfScope ps(PROF_GNN, s);
    static const int64_t CHUNK = [] {
        const char *e = getenv("CSPLAT_EM_CHUNK_ROWS");
        const int64_t v = e ? atoll(e) : 0;
        return (v >= 64 && v % 64 == 0 && v <= ((int64_t)1 << 22)) ? v : (int64_t)1 << 22;
    }();
    for (int64_t r0 = 0; r0 < M; r0 += CHUNK) {
        const int64_t rows = M - r0 < CHUNK ? M - r0 : CHUNK;
        const int64_t nst = (rows + 63) / 64;
        const int grid = (int)(nst < 256 ? nst : 256);      // persistent: one 4-wave workgroup per CU, two 32-row tiles in flight each
        unsigned long long *stamps = csplat_stamp_buffer((size_t)256 * 64);
        k_edge_mlp3r<F16, MODE><<<grid, 256, ErCfg<F16>::LDS_BYTES, s>>>(
            rows, e0 + r0 * in_cols, alpha, e0_absmax, xa, ia ? ia + r0 : nullptr, xb, ib ? ib + r0 : nullptr, (const i32x4 *)image, b0, b1, b2,
            gamma, beta, eps, out ? out + r0 * EM_N : nullptr, group_piece0 ? group_piece0 + r0 / 8 : nullptr, pieces, MODE == 2 ? in_cols : 0, stamps);
        LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t csplat_gnn_edge_mlp3_image_bytes(void) { return ErCfg<false>::IMAGE_BYTES; }      // (the larger of the two)

extern "C" int csplat_gnn_edge_mlp3_pack(void *stream, const float *W0, int ld0, const float *W1, int ld1, const float *W2, int ld2, void *image) {
    CSPLAT_REQUIRE(W0 && W1 && W2 && image && ld0 >= EM_N && ld1 >= EM_N && ld2 >= EM_N, "csplat_gnn_edge_mlp3_pack: bad arguments");
    CSPLAT_REQUIRE(aligned16(image), "csplat_gnn_edge_mlp3_pack: the image must be 16-byte aligned");
    return by_mode([&](auto f16) {
        k_edge_mlp3r_pack<decltype(f16)::value><<<4 * 3 * 8, 64, 0, (hipStream_t)stream>>>(W0, ld0, W1, ld1, W2, ld2, (i32x4 *)image);
        LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int csplat_absmax(void *stream, int64_t n, const float *x, float *out) {
    CSPLAT_REQUIRE(n >= 0 && out && (n == 0 || x) && (n & 3) == 0 && aligned16(x), "csplat_absmax: n must be a multiple of 4, x 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(float), s));
    if (n == 0) return 0;
    const int64_t nb = (n / 4 + 255) / 256;
    k_absmax<<<(int)(nb < 2048 ? nb : 2048), 256, 0, s>>>(n / 4, (const float4 *)x, (unsigned *)out);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_gnn_edge_mlp3(void *stream, int64_t E, const float *e0, float alpha, const float *e0_absmax, const float *xa,
                                    const int64_t *index_a, const float *xb, const int64_t *index_b, const void *image, const float *b0,
                                    const float *b1, const float *b2, const float *ln_gamma, const float *ln_beta, float ln_eps, float *out,
                                    const int32_t *group_piece0, float *pieces) {
    const bool agg = pieces != nullptr;
    CSPLAT_REQUIRE(E >= 0 && (E == 0 || (e0 && xa && index_a && xb && index_b && image && b0 && b1 && b2 && ln_gamma && ln_beta && (out || agg))),
                   "csplat_gnn_edge_mlp3: bad arguments");
    CSPLAT_REQUIRE(!agg || (group_piece0 && g_em_mode == 0), "csplat_gnn_edge_mlp3: the fused aggregation needs group_piece0 and mode 0");
    if (E == 0) return 0;
    CSPLAT_REQUIRE(aligned16(e0, xa, xb, image, b0, b1, b2, ln_gamma, ln_beta, out, pieces), "csplat_gnn_edge_mlp3: operands must be 16-byte aligned");
    CSPLAT_REQUIRE(out != e0 && pieces != e0, "csplat_gnn_edge_mlp3: out must not alias e0 (rows are read ahead of the rows being written)");
    int ex = 0;
    const float m = frexpf(alpha, &ex);
    CSPLAT_REQUIRE(alpha > 0.f && m == 0.5f, "csplat_gnn_edge_mlp3: alpha must be a power of two (the edge scale 2^l)");
    auto run = [&](auto f16, auto mode) {      // MODE 1 (agg): messages summed per destination, pieces out; 0: message rows out
        return em_launch_chunks<decltype(f16)::value, decltype(mode)::value>(
            (hipStream_t)stream, "csplat_gnn_edge_mlp3: 141 KB of dynamic LDS refused by the runtime", E, e0, EM_N, alpha, e0_absmax, xa, index_a, xb,
            index_b, image, b0, b1, b2, ln_gamma, ln_beta, ln_eps, out, group_piece0, pieces);
    };
    if (agg) return run(std::true_type{}, int_c<1>{});
    return by_mode([&](auto f16) { return run(f16, int_c<0>{}); });
}

extern "C" size_t csplat_gnn_node_update_image_bytes(void) { return NB_IMAGE_BYTES; }

// one launch of a PieceChain kernel over N rows (a 32-row tile per workgroup), KERNEL(N, args...)
template <auto KERNEL, class... A> static int chain_launch(void *stream, const char *lds_refused, int64_t N, A... args) {
    if (const int e = need_lds<KERNEL>(NB_LDS_BYTES, lds_refused)) return e;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_GNN, s);
    KERNEL<<<(unsigned)((N + 31) / 32), 256, NB_LDS_BYTES, s>>>(N, args...);
    LAUNCH_CHECK();
    return 0;
}

// k_node_pack under the current mode (absent matrices: nullptr, their slots are left as they are)
static int node_pack(void *stream, const float *W0, const float *W1, const float *W2, const float *W3, const float *W4, const float *W5, void *image) {
    return by_mode([&](auto f16) {
        k_node_pack<decltype(f16)::value><<<NB_MATS * 4 * 8, 64, 0, (hipStream_t)stream>>>(W0, W1, W2, W3, W4, W5, (i32x4 *)image);
        LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int csplat_gnn_node_update_pack(void *stream, const float *Wa, const float *Wx, const float *W2, const float *W3, const float *Wi_next,
                                           const float *Wj_next, void *image) {
    CSPLAT_REQUIRE(Wa && Wx && W2 && W3 && image && (Wi_next == nullptr) == (Wj_next == nullptr), "csplat_gnn_node_update_pack: bad arguments");
    CSPLAT_REQUIRE(aligned16(image), "csplat_gnn_node_update_pack: the image must be 16-byte aligned");
    return node_pack(stream, Wa, Wx, W2, W3, Wi_next, Wj_next, image);
}

extern "C" int csplat_gnn_node_update_packed(void *stream, int64_t N, const float *agg, const float *x, const void *image, const float *b0,
                                             const float *b2, const float *b3, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                             int has_next, float *x_new, float *xa_next, float *xb_next, const int32_t *piece_ptr) {
    CSPLAT_REQUIRE(N >= 0 && (N == 0 || (agg && x && image && b0 && b2 && b3 && ln_gamma && ln_beta && x_new)), "csplat_gnn_node_update_packed: bad arguments");
    CSPLAT_REQUIRE(!has_next || (xa_next && xb_next), "csplat_gnn_node_update_packed: next-layer outputs missing");
    CSPLAT_REQUIRE(x_new != x && x_new != agg, "csplat_gnn_node_update_packed: x_new must not alias an input (the residual reads x)");
    CSPLAT_REQUIRE(aligned16(agg, x, image, b0, b2, b3, ln_gamma, ln_beta, x_new, xa_next, xb_next), "csplat_gnn_node_update_packed: operands must be 16-byte aligned");
    if (N == 0) return 0;
    return by_mode([&](auto f16) {
        return chain_launch<k_node_update_b3<decltype(f16)::value>>(stream, "csplat_gnn_node_update_packed: 78 KB of dynamic LDS refused by the runtime", N, agg, x,
                                                                    (const i32x4 *)image, b0, b2, b3, ln_gamma, ln_beta, ln_eps, has_next ? 1 : 0, x_new,
                                                                    xa_next, xb_next, piece_ptr);
    });
}

// MODE 2 of the same kernel as a stand-alone operator: out[m] = LayerNorm( W2 relu( W1 relu( W0 x[m] + b0 ) + b1 ) + b2 ) for NARROW input rows
// x [M][K] (K a multiple of 4, <= 128): the encoders' MLPs (/root/reference/meshnet/graph_network.py:48-111) in one launch.  `image` =
// csplat_gnn_edge_mlp3_pack of (W0 padded with zero columns to [128][128], W1, W2) under mode 0; x_absmax as e0_absmax there.
extern "C" int csplat_gnn_mlp3_rows(void *stream, int64_t M, const float *x, int K, const float *x_absmax, const void *image, const float *b0,
                                    const float *b1, const float *b2, const float *ln_gamma, const float *ln_beta, float ln_eps, float *out) {
    CSPLAT_REQUIRE(M >= 0 && K >= 4 && K <= 128 && K % 4 == 0 && (M == 0 || (x && image && b0 && b1 && b2 && ln_gamma && ln_beta && out)),
                   "csplat_gnn_mlp3_rows: bad arguments (K a multiple of 4, 4 .. 128)");
    CSPLAT_REQUIRE(g_em_mode == 0, "csplat_gnn_mlp3_rows: mode 0 (fp16 pieces) only");
    if (M == 0) return 0;
    CSPLAT_REQUIRE(aligned16(x, image, b0, b1, b2, ln_gamma, ln_beta, out), "csplat_gnn_mlp3_rows: operands must be 16-byte aligned");
    return em_launch_chunks<true, 2>((hipStream_t)stream, "csplat_gnn_mlp3_rows: 141 KB of dynamic LDS refused by the runtime", M, x, K, 1.0f, x_absmax,
                                     nullptr, nullptr, nullptr, nullptr, image, b0, b1, b2, ln_gamma, ln_beta, ln_eps, out, nullptr, nullptr);
}

// ---- csplat_gnn_rows_chain: k_rows_chain (above).  mode 0: out_a = x Wa^T, out_b = x Wb^T; mode 1: out_a = relu(W1 relu(W0 x + b0) + b1).
// The image (csplat_gnn_node_update_image_bytes bytes) is packed under the current csplat_gnn_edge_mlp3_mode and must be used under it.
extern "C" int csplat_gnn_rows_chain_pack(void *stream, int mode, const float *Wfirst, const float *Wsecond, void *image) {
    CSPLAT_REQUIRE((mode == 0 || mode == 1) && Wfirst && Wsecond && image && aligned16(image), "csplat_gnn_rows_chain_pack: bad arguments");
    return node_pack(stream, Wfirst, mode == 0 ? Wsecond : nullptr, mode == 1 ? Wsecond : nullptr, nullptr, nullptr, nullptr, image);
}
extern "C" int csplat_gnn_rows_chain(void *stream, int64_t N, int mode, const float *x, const void *image, const float *b0, const float *b1,
                                     float *out_a, float *out_b) {
    CSPLAT_REQUIRE(N >= 0 && (mode == 0 || mode == 1) && (N == 0 || (x && image && out_a)) && (mode == 1 || out_b || N == 0),
                   "csplat_gnn_rows_chain: bad arguments");
    CSPLAT_REQUIRE(out_a != x && out_b != x, "csplat_gnn_rows_chain: the outputs must not alias x");
    CSPLAT_REQUIRE(aligned16(x, image, b0, b1, out_a, out_b), "csplat_gnn_rows_chain: operands must be 16-byte aligned");
    if (N == 0) return 0;
    auto run = [&](auto f16, auto md) {
        return chain_launch<k_rows_chain<decltype(f16)::value, decltype(md)::value>>(stream, "csplat_gnn_rows_chain: 78 KB of dynamic LDS refused by the runtime", N, x,
                                                                                    (const i32x4 *)image, b0, b1, out_a, out_b);
    };
    return by_mode([&](auto f16) { return mode == 0 ? run(f16, int_c<0>{}) : run(f16, int_c<1>{}); });
}
