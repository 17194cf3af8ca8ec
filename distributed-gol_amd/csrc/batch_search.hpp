// batch_search.hpp -- gol_batch_search<W, R, Rule>: a soup search without board memory, shared by
// the per-functor translation units batch_search_*.hip.  One workgroup per soup: it generates the
// board of the soup's seed in registers, runs it from generation 0 with gol_batch_period's cycle
// detection (batch_period.hpp: Brent, snapshots at turns 2^j - 1) until the soup repeats or
// max_turns have run, and writes one 32-byte record.  A soup that has repeated is retired: its
// workgroup ends and the CU takes the next soup of the grid.
//
// Seeding.  Lane (segment sg, column c16) holds rows sg R .. sg R + R - 1, word c16 & (wd - 1), as
// in gol_batch; init_random_word (golhip_internal.hpp) gives that word of the board of seed_i, bit
// for bit what batch_init_random stores there.  The snapshot starts as the board: gol_batch_period's
// t0 == 0 case, so the turn is the plain generation counter.
//
// Generations, snapshot, match mask: gol_batch_period's, without HIST.  sums16 and board_gen with the
// functor of period_next<Rule>; the snapshot moves one bit east per generation and is refreshed
// after turns 2^j - 1; a lane sets bit (g mod 32) of m when all its rows matched at generation g;
// every 32 generations (group 8 j + 7) and at the end put_mask reduces m over the wave into
// pm[block parity][w]; wave 0 reads the W masks one group later (take_mask, group 8 j + 8), ordered
// by that group's four barriers.
//
// Retirement.  When take_mask finds the first repeat, wave 0 stores 1 to `stop` (LDS).  EVERY wave
// reads `stop` at the end of the groups 8 j + 1, and leaves the generation loop there if it is set.
// board_gen has one workgroup barrier per generation, so a wave that left a generation earlier or
// later than the others would hang the workgroup; the exit is simultaneous because
//   - the points at which `stop` is read are a function of the group index alone, the same in
//     every wave;
//   - every wave reads the same value at such a point.  `stop` is written only by wave 0, at the
//     start (0) and at the end of a group 8 j (take_mask), before wave 0 enters the four barriers
//     of group 8 j + 1; lds_barrier waits lgkmcnt(0) first, so the store has landed when wave 0
//     arrives at the first of them, and no wave passes it before.  The read at the end of group
//     8 j + 1 is therefore after the store in every wave.  The next store to `stop` would come at
//     the end of group 8 j + 8, behind 24 more barriers which no wave passes before every wave has
//     done its read of group 8 j + 1 (the value is waited for and made wave-uniform with
//     readfirstlane at once, before the branch);
//   - the value only goes from 0 to 1.
// So either all waves leave at the end of group 8 j + 1, after 32 j + 8 generations, or none does.
// A repeat at turn r lies in block (r - 1) / 32 = j - 1: the soup stops after
// f(r) = 32 ((r - 1) / 32) + 40 generations, r + 8 <= f(r) <= r + 39, or at max_turns if that is
// less (golhip.h documents this function): the group loop and the 0..3 remainder end at
// max_turns exactly as gol_batch_period's end at K, with its end-of-launch put_mask, barrier and
// take_mask for a repeat in the last, partial block.  No mask is pending at an early exit: the
// block put at group 8 j - 1 was taken at group 8 j, the next put is at group 8 j + 7.
//
// Record.  After the loop each lane counts its alive cells under cmask (one copy of the board's
// row), wave_sum_dpp reduces them, lane 63 puts the wave's sum into LDS before the closing
// barrier, and lane 63 of wave 0 adds the W sums and stores the record with ordinary stores.
// Nothing is stored in board layout, so there is no unrotate16.
#pragma once
#include "batch_period.hpp"

namespace golhip {
namespace {

template <int W, int R, class Rule>
__global__ __launch_bounds__(64 * W) void gol_batch_search(BatchSearchParams sp) {
    constexpr int NSEG = 4 * W;
    __shared__ uint32_t ex[2][NSEG][4][16];
    __shared__ uint32_t pm[2][16];
    __shared__ uint32_t pop[16];
    __shared__ uint32_t stop;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = sp.wd;
    const int K = sp.max_turns;
    // one copy of the BOARD's row, as gol_batch's HIST counts it
    const int cw = (sp.width + 31) >> 5;
    const uint32_t cmask = c16 >= cw ? 0u : (c16 == cw - 1 && (sp.width & 31)) ? (1u << (sp.width & 31)) - 1u : ~0u;
    RuleMasks rm = sp.rule;
    if constexpr (!std::is_same_v<Rule, LifeNext>) {
        if (sp.rules) {  // the soup's own pair (a scalar load: blockIdx.x is wave-uniform)
            rm.birth = sp.rules[2 * (int64_t)blockIdx.x];
            rm.survive = sp.rules[2 * (int64_t)blockIdx.x + 1];
        }
    }
    const auto next = period_next<Rule>(rm);
    const uint64_t seed = sp.seeds ? sp.seeds[blockIdx.x] : sp.seed0 + (uint64_t)blockIdx.x;
    if (threadIdx.x == 0) stop = 0;
    uint32_t c[R], sn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = init_random_word(seed, sg * R + r, c16 & (wd - 1), sp.width, sp.density);
#pragma unroll
    for (int r = 0; r < R; ++r) sn[r] = c[r];  // board(0) is the first snapshot
    uint32_t m = 0;  // bit g % 32: every row of this lane matched the snapshot at generation g
    int rep = -1;    // wave 0: the first repeat turn
    const int up = (sg + NSEG - 1) % NSEG, dn = (sg + 1) % NSEG;
    // generation g (exchange buffer par): the rows advance in place
    auto gen = [&](int g, int par) {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16<R>(c, s, cy, ctr);
        board_gen<R>(s, cy, ctr, ex, par, sg, up, dn, c16, next, nx);
        uint32_t wl[R], acc = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) wl[r] = west16(sn[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) sn[r] = __builtin_amdgcn_alignbit(sn[r], wl[r], 31);  // one bit east
#pragma unroll
        for (int r = 0; r < R; ++r) acc = GOL_BOP3(acc, nx[r], sn[r], GOL_TT(a | (b ^ c)));
        if (acc == 0) m |= 1u << (g & 31);
        // pin the compare to its generation (see gol_batch)
        asm volatile("" : "+v"(m));
        // this generation completes turn g + 1; after turn 2^j - 1 the snapshot is the new board
        const uint32_t t1 = (uint32_t)g + 2;  // the turn + 1
        if ((t1 & (t1 - 1)) == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) sn[r] = nx[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = nx[r];
    };
    // the wave's match mask of block blk (generations [32 blk, 32 blk + 32)) to LDS
    auto put_mask = [&](int blk) {
        const uint32_t v = wave_and_dpp(m);
        if (lane == 63) pm[blk & 1][w] = v;
        m = 0;
    };
    // wave 0: the W masks of block blk, ordered by a barrier since put_mask; the first repeat
    // retires the soup
    auto take_mask = [&](int blk) {
        if (w == 0) {
            uint32_t v = pm[blk & 1][c16 & (W - 1)];
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x112, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x114, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x118, 0xf, 0xf, false);
            // lane 15 holds the AND of the row's 16 lanes: every wave's mask, W | 16
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
            if (all != 0 && rep < 0) {
                rep = 32 * blk + __builtin_ctz(all) + 1;
                if (lane == 0) stop = 1;
            }
        }
    };
    int g = 0, grp = 0;
    int pend = -1;  // the block whose masks lie in LDS, not yet taken by wave 0
    bool retired = false;
#pragma clang loop unroll(disable)
    while (g + 4 <= K) {
        gen(g, 0);
        gen(g + 1, 1);
        gen(g + 2, 0);
        gen(g + 3, 1);
        g += 4;
        if (pend >= 0) {
            take_mask(pend);
            pend = -1;
        }
        if ((grp & 7) == 7) {
            pend = grp >> 3;
            put_mask(pend);
        }
        // the one exit: the same group in every wave, the same value in every wave (see above)
        if ((grp & 7) == 1 && __builtin_amdgcn_readfirstlane((int)stop) != 0) {
            retired = true;
            break;
        }
        ++grp;
    }
    if (!retired) {
        const int rem = K - g;  // 0..3 generations left: one more, partial, group
        if (rem > 0) {
            gen(g, 0);
            if (rem > 1) gen(g + 1, 1);
            if (rem > 2) gen(g + 2, 0);
            g = K;
            if (pend >= 0) {
                take_mask(pend);
                pend = -1;
            }
        }
        // the last block if it is a partial one (bits of generations not run stay 0; a full block
        // before it was taken by the group that followed it)
        if ((K & 31) != 0) {
            pend = (K - 1) >> 5;
            put_mask(pend);
        }
    }
    // the alive cells of board(g); one more barrier orders the waves' sums and the last masks
    uint32_t a = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) a += (uint32_t)__builtin_popcount(c[r] & cmask);
    a = wave_sum_dpp(a);
    if (lane == 63) pop[w] = a;
    lds_barrier();
    if (pend >= 0) take_mask(pend);
    if (w == 0) {
        uint32_t v = lane < W ? pop[lane] : 0u;
        v = wave_sum_dpp(v);
        if (lane == 63) {
            SoupRecord rec;
            rec.repeat_turn = rep;
            // t - s(t), s(t) = 2^floor(log2 t) - 1: the snapshot turn of the window t lies in
            rec.period = rep > 0 ? rep - ((1 << (31 - __builtin_clz((uint32_t)rep))) - 1) : -1;
            rec.stop_turn = g;
            rec.population = v;
            rec.reserved = 0;
            sp.out[blockIdx.x] = rec;
        }
    }
}

// Every shape of the table under one functor.
template <class Rule>
hipError_t launch_batch_search_as(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s) {
#define GOLHIP_X(WW, RR)                                                                                        \
    if (W == WW && R == RR) {                                                                                   \
        hipLaunchKernelGGL((gol_batch_search<WW, RR, Rule>), dim3((unsigned)nsoups), dim3(64 * WW), 0, s, sp); \
        return hipGetLastError();                                                                               \
    }
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

}  // namespace

// One functor per translation unit (the build compiles them side by side): the constant-folded
// kernels of catalogue rule (B, S), declared in golhip_internal.hpp as launch_batch_search_<B>_<S>.
#define GOLHIP_DEFINE_BATCH_SEARCH_CONST(B, S)                                                                        \
    hipError_t launch_batch_search_##B##_##S(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s) { \
        return launch_batch_search_as<RuleConst<(B), (S)>>(W, R, nsoups, sp, s);                                    \
    }

}  // namespace golhip
