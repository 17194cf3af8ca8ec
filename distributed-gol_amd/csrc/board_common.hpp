// board_common.hpp -- the whole-torus-in-one-workgroup geometry: its device helpers, the (W waves,
// R rows per segment) table, the one generation step (board_gen) behind gol_board
// (stencil_board.hip: one board per launch), gol_batch (batch_board.hip) and gol_batch_rule
// (batch_rule.hpp): one board per workgroup of the grid.
//
// Layout: a wave's 64 lanes are four 16-lane DPP rows ("segments"); segment sg = 4 w + (lane / 16)
// holds board rows [sg R, sg R + R), one row per VGPR, lane l % 16 holding word (l % 16) % wd of
// the row -- a row of wd in {4, 8, 16} words is replicated to 16 lanes (the torus evolution keeps
// the horizontal period).  The west neighbour word is DPP row_ror:1 (the torus wrap inside the
// 16-lane row).
#pragma once
#include "stencil_tile.hpp"

namespace golhip {
namespace {

__device__ __forceinline__ uint32_t west16(uint32_t v) {  // lane l <- lane (l - 1) mod 16 of its row
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121 /* row_ror:1 */, 0xf, 0xf, false);
}

// Drifting 3-cell sums of N rows, op-major (sums_om with the 16-lane torus wrap).
template <int N>
__device__ __forceinline__ void sums16(const uint32_t (&x)[N], uint32_t (&s)[N], uint32_t (&cy)[N],
                                       uint32_t (&ctr)[N]) {
    uint32_t wl[N], w2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) wl[i] = west16(x[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) ctr[i] = __builtin_amdgcn_alignbit(x[i], wl[i], 31);  // cell x-1 onto x
#pragma unroll
    for (int i = 0; i < N; ++i) w2[i] = __builtin_amdgcn_alignbit(x[i], wl[i], 30);  // cell x-2 onto x
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = GOL_BOP3(w2[i], ctr[i], x[i], kXor3);
#pragma unroll
    for (int i = 0; i < N; ++i) cy[i] = GOL_BOP3(w2[i], ctr[i], x[i], kMaj);
}

// The word of a drifted row (K bits east around the replicated 512-bit torus) rotated back: bits
// [32 j + K, 32 j + K + 32) of the 16-lane row, for lane j of the row.
__device__ __forceinline__ uint32_t unrotate16(uint32_t v, int lane, int K) {
    const int base = lane & ~15, j = lane & 15, q = (K >> 5) & 15, r = K & 31;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((base + ((j + q) & 15)) << 2, (int)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((base + ((j + q + 1) & 15)) << 2, (int)v);
    return __builtin_amdgcn_alignbit(hi, lo, r);
}

// wave_sum_dpp of N values at once (the six DPP steps interleaved over the N independent sums)
template <int N>
__device__ __forceinline__ void wave_sum_dpp_n(uint32_t (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x111, 0xf, 0xf, false);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x112, 0xf, 0xf, false);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x114, 0xf, 0xf, false);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x118, 0xf, 0xf, false);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x142, 0xa, 0xf, false);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], 0x143, 0xc, 0xf, false);
}

// (W, R) by board height, first match: 4 W R == height.  16 waves while the rows allow (4 per SIMD
// hide the VALU latency of each wave's R independent rows), then fewer.
#define GOLHIP_BOARD_SHAPES(X) X(16, 8) X(16, 4) X(8, 4) X(4, 4) X(2, 4) X(1, 4) X(1, 2) X(1, 1)

// The workgroup barrier of a generation: it orders LDS traffic only, so it waits for lgkmcnt and
// leaves the global loads and stores in flight.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// B3/S23 as board_gen's rule step.
struct LifeNext {
    template <int N>
    __device__ __forceinline__ void operator()(const uint32_t (&as)[N], const uint32_t (&acy)[N],
                                               const uint32_t (&ms)[N], const uint32_t (&mcy)[N],
                                               const uint32_t (&mc)[N], const uint32_t (&bs)[N],
                                               const uint32_t (&bcy)[N], uint32_t (&out)[N]) const {
        life_om<N>(as, acy, ms, mcy, mc, bs, bcy, out, AllRows{});
    }
};

// One generation of segment sg's R rows from their sums16 (s, cy, ctr): nx = the next generation,
// one bit further east.  The caller runs sums16 itself and keeps ctr (the old rows in nx's frame,
// which SETTLE and gol_board's LD need): with sums16 in here and ctr handed back, the compiler
// ordered the loops of the SETTLE-only batch kernels differently and they ran 2-4 % slower; this
// way gol_batch and the catalogue kernels compile to the code they had with the step written out
// in each kernel.  A segment's edge rows need
// the sums of the segments above (up) and below (dn): every segment puts the sums of its own edge
// rows into ex[par], computes its interior rows while they travel, and reads its neighbours' after
// ONE LDS-only barrier.  ex is double-buffered by generation parity: a wave that is a generation
// ahead writes ex[par ^ 1], and cannot reach its next write of ex[par] before every wave has passed
// the barrier between -- after its reads of ex[par], which the barrier's lgkmcnt(0) completes.
// The rule enters only as next.template operator()<N>(as, acy, ms, mcy, mc, bs, bcy, out): the
// sums of the rows above, of the rows themselves with their centres, and of the rows below -> out.
template <int R, int NSEG, class Next>
__device__ __forceinline__ void board_gen(const uint32_t (&s)[R], const uint32_t (&cy)[R], const uint32_t (&ctr)[R],
                                          uint32_t (&ex)[2][NSEG][4][16], int par, int sg, int up, int dn, int c16,
                                          const Next &next, uint32_t (&nx)[R]) {
    ex[par][sg][0][c16] = s[0];
    ex[par][sg][1][c16] = cy[0];
    ex[par][sg][2][c16] = s[R - 1];
    ex[par][sg][3][c16] = cy[R - 1];
    if constexpr (R >= 3) {  // the interior rows from the segment's own sums
        constexpr int NI = R - 2;
        uint32_t as[NI], acy[NI], ms[NI], mcy[NI], mc[NI], bs[NI], bcy[NI], ni[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            as[i] = s[i], acy[i] = cy[i];
            ms[i] = s[i + 1], mcy[i] = cy[i + 1], mc[i] = ctr[i + 1];
            bs[i] = s[i + 2], bcy[i] = cy[i + 2];
        }
        next.template operator()<NI>(as, acy, ms, mcy, mc, bs, bcy, ni);
#pragma unroll
        for (int i = 0; i < NI; ++i) nx[i + 1] = ni[i];
    }
    lds_barrier();
    const uint32_t ts = ex[par][up][2][c16], tcy = ex[par][up][3][c16];  // the row above row 0
    const uint32_t bts = ex[par][dn][0][c16], btcy = ex[par][dn][1][c16];  // below row R - 1
    if constexpr (R == 1) {
        uint32_t as[1] = {ts}, acy[1] = {tcy}, ms[1] = {s[0]}, mcy[1] = {cy[0]}, mc[1] = {ctr[0]};
        uint32_t bs[1] = {bts}, bcy[1] = {btcy}, n1[1];
        next.template operator()<1>(as, acy, ms, mcy, mc, bs, bcy, n1);
        nx[0] = n1[0];
    } else {
        uint32_t as[2] = {ts, s[R - 2]}, acy[2] = {tcy, cy[R - 2]};
        uint32_t ms[2] = {s[0], s[R - 1]}, mcy[2] = {cy[0], cy[R - 1]}, mc[2] = {ctr[0], ctr[R - 1]};
        uint32_t bs[2] = {s[1], bts}, bcy[2] = {cy[1], btcy}, n2[2];
        next.template operator()<2>(as, acy, ms, mcy, mc, bs, bcy, n2);
        nx[0] = n2[0];
        nx[R - 1] = n2[1];
    }
}

}  // namespace
}  // namespace golhip
