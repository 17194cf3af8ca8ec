// board_common.hpp -- the device helpers of the whole-torus-in-one-workgroup geometry, shared by
// gol_board (stencil_board.hip: one board per launch) and gol_batch (batch_board.hip: one board per
// workgroup of the grid), and the (W waves, R rows per segment) table both use.
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

}  // namespace
}  // namespace golhip
