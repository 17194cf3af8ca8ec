// stencil_board.hip -- gol_board: the WHOLE board in one workgroup, for the reference's own sizes
// (boards at most 16 packed words = 512 cells wide and 512 rows tall: images/16x16 ... 512x512,
// configs[0]).
//
// Every other kernel splits a board over many workgroups and pays for it per launch: a K-row
// trapezoid of redundant rows at each slab edge (temporal blocking), halo lanes at each column
// chunk, and a launch boundary (dispatch ramp, row loads, tail: ~3 us) every K <= 16 generations.
// On a 512^2 board those launches are latency-bound (~0.5 us per generation whatever the shape,
// profiles/r04/r04p4_narrow_sweep.log) and the boundaries add ~30 %.  Here one workgroup holds
// the whole torus in registers for ALL the generations of a call (K is a runtime count, up to
// kBoardMaxK): no trapezoid, no halo lanes, no launch boundary inside a call, per-generation counts
// summed in LDS.
//
// Layout: a wave's 64 lanes are four 16-lane DPP rows ("segments"); segment sg = 4 w + (lane / 16)
// holds board rows [sg R, sg R + R), one row per VGPR, lane l % 16 holding word (l % 16) % wd of
// the row -- a row of wd in {4, 8, 16} words is replicated to 16 lanes (the torus evolution keeps
// the horizontal period).  The west neighbour word is DPP row_ror:1 (the torus wrap inside the
// 16-lane row), so there is no horizontal halo and no stale bit: the drifting sums of gol_stencil
// (one DPP + two v_alignbit + nine v_bitop3 per word per generation) move the whole row one bit east
// per generation around the torus, and the stores rotate it back by K bits at the end.  Vertical
// neighbours are the next VGPR of the same lane; a segment's edge rows' SUMS go through LDS to the
// segments above and below (double-buffered by generation parity, one LDS-only barrier per
// generation), as in gol_slab2: the interior rows are computed before the barrier.
// That generation step (board_gen), the lane layout's device helpers (west16, sums16, unrotate16,
// wave_sum_dpp_n) and the (W, R) table are in board_common.hpp, shared with gol_batch
// (batch_board.hip) and gol_batch_rule (batch_rule.hpp); this file adds the COUNT slots and LD flips.
#include "board_common.hpp"

namespace golhip {
namespace {

// W waves, R rows per segment: the board has exactly 4 W R rows.  COUNT: generation g's count of
// wave w into slots[g * kCountSlots + w] with a plain store from one lane (count_finalize sums the
// slots and re-zeroes them; W <= 16 < kCountSlots).  An LDS atomic per generation compiled to the
// atomic optimiser's lane loop plus a ds_add on the wave's critical path; the per-generation LDS
// array also capped K by the LDS size.  LD: the last generation's flips (gol/distributor.go:53-59)
// into p.diff.
template <int W, int R, bool COUNT, bool LD>
__global__ __launch_bounds__(64 * W) void gol_board(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                    StencilParams p, unsigned long long *__restrict__ slots,
                                                    int K) {
    constexpr int NSEG = 4 * W;
    __shared__ uint32_t ex[2][NSEG][4][16];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = p.wd;
    const bool own = c16 < wd;  // one copy of the replicated row stores and counts
    uint32_t c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = in[(int64_t)(sg * R + r) * p.pitch + c16 % wd];
    const int up = (sg + NSEG - 1) % NSEG, dn = (sg + 1) % NSEG;
    uint32_t dlast[LD ? R : 1];  // LD: the last generation's flips (drifted frame)
    // generation g (exchange buffer par = g & 1): the rows advance in place; returns this lane's
    // alive cells of the new generation (COUNT)
    auto gen = [&](int g, int par) -> uint32_t {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16<R>(c, s, cy, ctr);
        board_gen<R>(s, cy, ctr, ex, par, sg, up, dn, c16, LifeNext{}, nx);
        uint32_t a = 0;
        if constexpr (COUNT)
#pragma unroll
            for (int r = 0; r < R; ++r) a += (uint32_t)__builtin_popcount(own ? nx[r] : 0u);
        if constexpr (LD)
            if (g == K - 1)
#pragma unroll
                for (int r = 0; r < R; ++r) dlast[r] = nx[r] ^ ctr[r];  // same (new) frame
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = nx[r];
        return a;
    };
    // Generations in groups of 4: their four per-wave count reductions (6 dependent DPP adds each)
    // run interleaved after the group instead of one chain inside every generation.
    int g = 0;
#pragma clang loop unroll(disable)
    for (; g + 4 <= K; g += 4) {
        uint32_t a[4];
        a[0] = gen(g, 0);
        a[1] = gen(g + 1, 1);
        a[2] = gen(g + 2, 0);
        a[3] = gen(g + 3, 1);
        if constexpr (COUNT) {
            wave_sum_dpp_n<4>(a);
            if (lane == 63)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (a[u]) slots[(int64_t)(g + u) * kCountSlots + w] = a[u];  // vector stores (lane 63)
        }
    }
#pragma clang loop unroll(disable)
    for (; g < K; ++g) {
        uint32_t a = gen(g, g & 1);
        if constexpr (COUNT) {
            a = wave_sum_dpp(a);
            if (lane == 63 && a) slots[(int64_t)g * kCountSlots + w] = a;
        }
    }
    // the rows back in the board frame (K bits west around the torus), one copy stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = unrotate16(c[r], lane, K);
        if (own) out[(int64_t)(sg * R + r) * p.pitch + c16] = v;
        if constexpr (LD) {
            const uint32_t d = unrotate16(dlast[r], lane, K);
            if (own) p.diff[(int64_t)(sg * R + r) * p.pitch + c16] = d;
        }
    }
}

template <int W, int R>
hipError_t launch_board_wr(int K, const uint32_t *in, uint32_t *out, const StencilParams &p,
                           unsigned long long *slots, hipStream_t s) {
    if (p.diff && slots)
        hipLaunchKernelGGL((gol_board<W, R, true, true>), dim3(1), dim3(64 * W), 0, s, in, out, p, slots, K);
    else if (p.diff)
        hipLaunchKernelGGL((gol_board<W, R, false, true>), dim3(1), dim3(64 * W), 0, s, in, out, p, slots, K);
    else if (slots)
        hipLaunchKernelGGL((gol_board<W, R, true, false>), dim3(1), dim3(64 * W), 0, s, in, out, p, slots, K);
    else
        hipLaunchKernelGGL((gol_board<W, R, false, false>), dim3(1), dim3(64 * W), 0, s, in, out, p, slots, K);
    return hipGetLastError();
}

}  // namespace

bool stencil_board_shape(int64_t height, int32_t wd, int *W, int *R) {
    if (wd != 4 && wd != 8 && wd != 16) return false;  // 16 % wd == 0: the row replicates to 16 lanes
#define GOLHIP_X(WW, RR)                       \
    if (height == 4 * WW * RR) {               \
        if (W) *W = WW;                        \
        if (R) *R = RR;                        \
        return true;                           \
    }
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return false;
}

hipError_t launch_stencil_board(int K, int W, int R, const uint32_t *in_row0, uint32_t *out_row0,
                                const StencilParams &p, unsigned long long *slots, hipStream_t s) {
    if (K < 1 || K > kBoardMaxK || p.wrap_rows != (int64_t)4 * W * R) return hipErrorInvalidValue;
#define GOLHIP_X(WW, RR) \
    if (W == WW && R == RR) return launch_board_wr<WW, RR>(K, in_row0, out_row0, p, slots, s);
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

}  // namespace golhip
