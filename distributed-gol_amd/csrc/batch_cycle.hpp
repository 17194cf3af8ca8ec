// batch_cycle.hpp -- gol_batch_cycle<W, R, Rule>: the exact pass of golhip_batch_search_exact,
// instantiated by batch_cycle.hip.  It runs after the unchanged search kernel
// (gol_batch_search or gol_plane_search) on the same chunk, one workgroup per soup, reads the soup's
// record (repeat_turn, period) from the chunk's record buffer and writes cycle_start[soup]: the least
// t >= 0 with board(t + period) == board(t), -1 for a soup without a repeat.
//
// What the record gives.  repeat_turn = s + period with s = 2^j - 1 the snapshot turn: board(s) is
// on the cycle, so
//   0 <= cycle_start <= s = repeat_turn - period, and cycle_start + period <= repeat_turn <= max_turns:
//   the pass never needs a generation beyond repeat_turn;
//   cycle_start == 0 exactly when board(0) is on the cycle.
// The lower bound lo (golhip.cycle_start_floor).  If j > 0 and period <= 2^(j-1), the previous
// snapshot, at s' = 2^(j-1) - 1 with the window s' + 1 .. s, would have matched at s' + period <= s had
// the soup been on its cycle by s'; it did not (repeat_turn is the FIRST match), hence cycle_start >
// s' and lo = s'.  Otherwise nothing is known and lo = 0.  With s == 0, cycle_start is 0 and nothing
// runs.
//
// The run.
//   1. Board A is seeded as gol_plane_search seeds its board: init_random_word & box_word_mask (the
//      whole board when no box is set: the mask is all ones).
//   2. A alone runs lo generations.
//   3. B = A: board(lo).
//   4. A runs `period` more generations; B moves one bit east per generation with the snapshot mover
//      (west16 + v_alignbit), so the two keep one frame: A = board(lo + period), B = board(lo).
//   5. Lockstep, index i = 0 .. s - lo for turn t = lo + i: compare A with B, then step both.  The
//      first t at which every lane of the workgroup finds its rows equal is cycle_start.  Equality
//      of whole boards is monotone in t (the rule is deterministic), and it holds at t = s, so the
//      compare of i = s - lo always matches and is not followed by a step.
// Work: lo + period + 2 (cycle_start - lo) board generations plus the detection slack below, never
// above about 1.5 s + period.
//
// One kernel for torus and plane.  The plane switch is the run-time per-lane value of
// gol_plane_search: off, Z is all ones (and stays so) and up / dn wrap; on, Z is the seam mask of
// batch_plane.hpp and the exchange array's dead slot NSEG stands for the row beyond the top and the
// bottom.  A and B share a frame from step 3 on and therefore share Z: sums16_plane advances its
// argument in place, so in the lockstep both calls start from a copy of this generation's Z and Z
// advances once per generation.
//
// The exchange array.  A and B share ONE ex[2][NSEG + 1][4][16]; every board_gen call of the kernel,
// whichever board it steps, takes the parity opposite to the call before it (the call's index
// mod 2, from the loop counters: in the lockstep A and B alternate).  board_common.hpp's double-buffer argument speaks of consecutive
// CALLS, not of generations of one board, so it holds as it stands: call k writes ex[par], passes
// ONE barrier and reads ex[par]; a wave that is a call ahead writes ex[par ^ 1]; it reaches call
// k + 2's writes of ex[par] only through call k + 1's barrier, which no wave passes before every
// wave has arrived there -- after its reads of ex[par] of call k, which that barrier's lgkmcnt(0)
// completes.  The dead slot is written once, before the first barrier, in both halves.
//
// Detection and exit: gol_batch_search's machinery over lockstep indices.  A lane sets bit (i mod 32)
// of m when all its rows are equal at index i (pinned to that index by an empty asm); at the end of
// the iterations i = 32 k + 31 put_mask AND-reduces m over the wave (wave_and_dpp) into
// pm[k & 1][w]; wave 0 takes the W masks at the end of iteration 32 k + 32, ordered by that
// iteration's two barriers, and on the first nonzero AND records 32 k + ctz and stores 1 to `stop`
// (LDS); EVERY wave reads `stop` at the end of the iterations 32 k + 33 and leaves the loop there if
// it is set.
//
// The barrier argument.  Every iteration of the lockstep loop but the closing compare has two
// workgroup barriers (A's board_gen, B's board_gen), the solo loops one per generation; a wave that
// left a loop an iteration earlier or later than the others would hang the workgroup.
//   - The trip counts lo, period and n = s - lo + 1 come from the soup's record, loaded at an
//     address that depends on blockIdx.x only: wave-uniform and the same in every wave.  A soup
//     without a repeat, and one with s == 0 (unless an ash buffer is set: the ash hand-off below),
//     returns before its first barrier, in every wave.
//   - The points at which `stop` is read are a function of the index i alone.
//   - Every wave reads the same value there.  `stop` is written by thread 0 at the start (0, before
//     the first barrier; the first read follows at least two barriers) and by wave 0 in take_mask
//     at the end of iteration 32 k + 32, before wave 0 enters the two barriers of iteration
//     32 k + 33; lds_barrier waits lgkmcnt(0) first, so the store has landed when wave 0 arrives at
//     the first of them and no wave passes it before.  The read at the end of iteration 32 k + 33 is
//     after the store in every wave; the next store would come at the end of iteration 32 k + 64,
//     behind 60 more barriers that no wave passes before every wave has done its read (the value is
//     made wave-uniform with readfirstlane at once, before the branch).
//   - The value only goes from 0 to 1.
//   So all waves leave at the end of iteration 32 k + 33 or none does.  No mask is pending then: the
//   block put at 32 k + 31 was taken at 32 k + 32 and the next put is at 32 k + 63.  An iteration
//   32 k + 33 that is the closing compare (no barriers) is outside the loop and reads nothing.
//   - The hard bound: the loop ends at i = n - 1 whatever the flag says, so the pass terminates
//     without it; the closing compare, put_mask of its block, ONE barrier and the remaining takes
//     (the block put at n - 2 if it was one, then the closing block) give the answer, as
//     gol_batch_search's end of launch does.  pm's parity is safe as there: block k + 2 overwrites
//     pm[k & 1] more than 60 barriers after wave 0 read it, and the two takes at the end are of
//     adjacent blocks.
// cycle_start = lo + the first index, stored by lane 0 of wave 0 with an ordinary store.
//
// The ash hand-off (golhip_batch_search_census).  With cp.ash set the workgroup also stores a board
// that lies on the soup's cycle, for the census that follows on the same stream, and its turn:
//   - a soup that repeated, s > 0: board A as it leaves the lockstep -- by the flag or by the closing
//     compare -- at turn T = the generations A has run: lo + period alone, then one per lockstep
//     index whose step ran.  A was seeded at drift 0 and drifts one bit east per generation, so the
//     rows go back to the board frame as gol_plane_rule's and gol_batch_period's do: unrotate16(a[r],
//     lane, T & 511), one copy of the replicated row stored by the lanes c16 < wd.  Z plays no part.
//     cycle_start <= lo + first < T on the flag exit and T = repeat_turn on the closing compare; the
//     loop stops before index n - 1, so T <= lo + period + n - 1 = repeat_turn either way: board T
//     is on the cycle and no generation beyond repeat_turn has run.  T is a function of the record
//     and of cycle_start alone: the flag exit is at index 32 (first / 32) + 33 if that is below
//     n - 1, the closing compare otherwise.  The ash is NOT phase-aligned to cycle_start: that would
//     take another inlined copy of the step.
//   - s <= 0 (board(0) is on the cycle): the seeded board, T = 0.  The early return is taken only
//     without an ash buffer; with one the workgroup runs on with every trip count zero (no solo
//     generation, no lockstep iteration), the closing compare finds A == B = board(0) and gives
//     cycle_start = 0, and the store site below is the only one.
//   - no repeat: ash_turn = -1 and no row; the host has zeroed the chunk's buffer.
// cp.ash is a kernel argument, workgroup-uniform: whether the s <= 0 workgroup returns early (before
// its first barrier, in every wave) or runs on (through the closing compare's ONE barrier, in every
// wave) is the same in all its waves.  The tail itself has no barrier: it comes after the last
// one, adds one ds_bpermute pair and one store per row, and every wave reaches it with the same T
// (solo, i and the exit taken are wave-uniform and the same in every wave, see above).  With
// cp.ash null the kernel writes what it always wrote.
//
// Functors: LifeNext for a uniform B3/S23, RuleNext<RuleTable> for every other rule, per-soup rules
// included: 8 shapes x 2 kernels.  A catalogue rule (HighLife, ...) whose search ran constant-folded
// runs this pass in the table form; the results are the rule's, not the form's.
#pragma once
#include "batch_plane.hpp"

namespace golhip {
namespace {

template <int W, int R, class Rule>
__global__ __launch_bounds__(64 * W) void gol_batch_cycle(BatchCycleParams cp) {
    constexpr int NSEG = 4 * W;
    const BatchSearchParams &sp = cp.bp.s;
    __shared__ uint32_t ex[2][NSEG + 1][4][16];
    __shared__ uint32_t pm[2][16];
    __shared__ uint32_t stop;
    // the soup's record (scalar loads: blockIdx.x is wave-uniform); all exits here are before the
    // first barrier and the same in every wave
    const int rep = __builtin_amdgcn_readfirstlane((int)sp.out[blockIdx.x].repeat_turn);  // <= 2^20
    const int period = __builtin_amdgcn_readfirstlane((int)sp.out[blockIdx.x].period);
    if (rep < 0) {
        if (threadIdx.x == 0) {
            cp.cycle_start[blockIdx.x] = -1;
            if (cp.ash) cp.ash_turn[blockIdx.x] = -1;  // no ash: the host has zeroed the chunk
        }
        return;
    }
    const int s = rep - period;  // the snapshot turn 2^j - 1
    // board(0) is on the cycle: nothing runs.  Without an ash buffer the workgroup leaves here, as it
    // always did; with one (a kernel argument: the same in every wave) it goes on with every trip
    // count zero, seeds board(0) below, finds it equal to itself in the closing compare and stores
    // it at the one store site, turn 0.
    const bool still = s <= 0;
    if (still && !cp.ash) {
        if (threadIdx.x == 0) cp.cycle_start[blockIdx.x] = 0;
        return;
    }
    const int half = (s + 1) >> 1;                // 2^(j-1)
    const int lo = period <= half ? half - 1 : 0;  // cycle_start_floor
    const int solo = still ? 0 : lo + period;     // A's generations before the lockstep
    const int n = still ? 1 : s - lo + 1;          // lockstep compares: turns lo .. s
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = sp.wd;
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
    plane_zero_slot<NSEG>(ex);
    // a torus: no seam mask, and the segments wrap
    const bool plane = cp.bp.plane != 0;
    uint32_t Z = plane ? plane_z0(sp.width, c16) : ~0u;
    uint32_t a[R], b[R];
    // the soup of the seed with every cell outside the box cleared, as gol_plane_search seeds it
#pragma unroll
    for (int r = 0; r < R; ++r)
        a[r] = init_random_word(seed, sg * R + r, c16 & (wd - 1), sp.width, sp.density) &
               box_word_mask(sg * R + r, c16 & (wd - 1), sp.width, cp.bp.box);
    const int up = sg == 0 ? (plane ? NSEG : NSEG - 1) : sg - 1;
    const int dn = sg == NSEG - 1 ? (plane ? NSEG : 0) : sg + 1;
    // one generation of board x under seam mask z (advanced in place) through exchange buffer par:
    // call k of the kernel, whichever board it steps, takes par = k & 1.  The callers derive it from
    // their loop counters; carried from call to call in a variable of its own it was moved to the
    // vector unit once the ash tail stood behind the loops, a v_mul_lo_u32 per call for ex[par].
    auto gen = [&](uint32_t(&x)[R], uint32_t &z, int par) {
        uint32_t sm[R], cy[R], ctr[R], nx[R];
        sums16_plane<R>(x, z, sm, cy, ctr);
        board_gen<R>(sm, cy, ctr, ex, par, sg, up, dn, c16, next, nx);
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] = nx[r];
    };
    // 2. - 4. in one loop (one copy of the step in the code object): A alone to board(lo), B = A
    // there, then A to board(lo + period) with B one bit east per generation.  The two branches are
    // workgroup-uniform (lo comes from the record).
#pragma unroll
    for (int r = 0; r < R; ++r) b[r] = a[r];
#pragma clang loop unroll(disable)
    for (int g = 0; g < solo; ++g) {
        if (g == lo) {
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = a[r];
        }
        gen(a, Z, g & 1);
        if (g >= lo) {
            uint32_t wl[R];
#pragma unroll
            for (int r = 0; r < R; ++r) wl[r] = west16(b[r]);
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = __builtin_amdgcn_alignbit(b[r], wl[r], 31);  // one bit east
        }
    }
    uint32_t m = 0;  // bit i % 32: every row of this lane was equal at lockstep index i
    int first = -1;  // wave 0: the first index at which the boards were equal
    auto compare = [&](int i) {
        uint32_t acc = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) acc = GOL_BOP3(acc, a[r], b[r], GOL_TT(a | (b ^ c)));
        if (acc == 0) m |= 1u << (i & 31);
        // pin the compare to its index (see gol_batch)
        asm volatile("" : "+v"(m));
    };
    // the wave's mask of block blk (indices [32 blk, 32 blk + 32)) to LDS
    auto put_mask = [&](int blk) {
        const uint32_t v = wave_and_dpp(m);
        if (lane == 63) pm[blk & 1][w] = v;
        m = 0;
    };
    // wave 0: the W masks of block blk, ordered by a barrier since put_mask; the first equality
    auto take_mask = [&](int blk) {
        if (w == 0) {
            uint32_t v = pm[blk & 1][c16 & (W - 1)];
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x112, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x114, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x118, 0xf, 0xf, false);
            // lane 15 holds the AND of the row's 16 lanes: every wave's mask, W | 16
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
            if (all != 0 && first < 0) {
                first = 32 * blk + __builtin_ctz(all);
                if (lane == 0) stop = 1;
            }
        }
    };
    // 5. the lockstep: indices 0 .. n - 2 compare and step, index n - 1 only compares
    int i = 0;
    int pend = -1;  // the block whose masks lie in LDS, not yet taken by wave 0
    bool retired = false;
#pragma clang loop unroll(disable)
    while (i < n - 1) {
        compare(i);
        // A, then B: ONE copy of the step in the code object (the library has a size to keep), run
        // twice with the boards swapped after each run -- 2 R moves per run against the step's
        // ~40 R VALU.  Both runs start from this generation's Z (sums16_plane advances its argument
        // in place); the second run's result is the next generation's.
        uint32_t zn = Z;
#pragma clang loop unroll(disable)
        for (int h = 0; h < 2; ++h) {
            zn = Z;
            gen(a, zn, (solo ^ h) & 1);  // two calls per index: the parity the solo loop left, then the other
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t t = a[r];
                a[r] = b[r];
                b[r] = t;
            }
        }
        Z = zn;
        if (pend >= 0) {
            take_mask(pend);
            pend = -1;
        }
        if ((i & 31) == 31) {
            pend = i >> 5;
            put_mask(pend);
        }
        // the one exit: the same index in every wave, the same value in every wave (see above)
        if ((i & 31) == 1 && __builtin_amdgcn_readfirstlane((int)stop) != 0) {
            retired = true;
            break;
        }
        ++i;
    }
    if (!retired) {
        compare(n - 1);  // turn s: equal by the record
        const int last = (n - 1) >> 5;
        put_mask(last);
        lds_barrier();
        if (pend >= 0) take_mask(pend);
        take_mask(last);
    }
    if (threadIdx.x == 0) cp.cycle_start[blockIdx.x] = first >= 0 ? (int64_t)lo + first : -1;
    // The ash: board A as it left the lockstep, back in the board frame.  A has run `solo` generations
    // alone and one per lockstep index passed: i of them when the loop ran out (the closing compare
    // steps nothing), i + 1 when the flag ended it behind index i's step.
    if (cp.ash) {
        const int T = __builtin_amdgcn_readfirstlane(solo + i + (retired ? 1 : 0));
        // The tail's lane arithmetic starts from a thread index the compiler cannot see through: taken
        // from lane, c16 and sg above it is loop-invariant, and its addresses were computed before the
        // loops and held in registers through them (the (16, 8) kernels went from 59 to 71 VGPRs and
        // from 8 to 7 waves per SIMD: one workgroup per CU instead of two).
        int tid = (int)threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int tl = tid & 63, tc = tid & 15, ts = tid >> 4;  // lane, c16, sg
        const bool own = tc < wd;  // one copy of the replicated row is stored
        uint32_t *__restrict__ board = cp.ash + (int64_t)blockIdx.x * (NSEG * R) * wd;  // board_pitch: height * wd
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t v = unrotate16(a[r], tl, T & 511);
            if (own) board[(ts * R + r) * wd + tc] = v;
        }
        if (threadIdx.x == 0) cp.ash_turn[blockIdx.x] = T;
    }
}

// Every shape of the table under one functor.
template <class Rule>
hipError_t launch_batch_cycle_as(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s) {
#define GOLHIP_X(WW, RR)                                                                                       \
    if (W == WW && R == RR) {                                                                                  \
        hipLaunchKernelGGL((gol_batch_cycle<WW, RR, Rule>), dim3((unsigned)nsoups), dim3(64 * WW), 0, s, cp); \
        return hipGetLastError();                                                                              \
    }
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace golhip
