// batch_census.hpp -- gol_batch_census: the census of every board of a batch by bit-parallel template
// matching (golhip_batch_census, include/golhip.h states the definitions).  ONE kernel: width, height,
// topology and the pattern table are run-time values.  It steps no generation, so it needs none of
// the (W, R) register tilings of the stepping kernels, and the production library has a size to
// keep (tests/test_boundary.py).
//
// One workgroup per board, blockIdx.x = the board within the launch, in four phases.
//
// 1. The frame.  The board is staged once in dynamic LDS as FR = height + 62 rows of FW = nw + 2 words,
//    nw = max(1, width / 32) the words that hold one copy of a row: 31 margin rows above and below
//    and one margin word left and right, filled with the wrapped cells on a torus and with zeros on
//    a plane.  A row narrower than a word holds 32 / width replicas in its word: on a torus they are
//    exactly the wrap, on a plane the bits at columns >= width are cleared.  After this the match loop
//    does not know the topology: it only starts at another anchor row and word group (a torus has
//    no negative anchors).
// 2. The match.  A lane owns 32 consecutive anchors of one anchor row: bit b of its match word is
//    the anchor at bit b of frame word g, and cell (r, c) of the pattern lies at bit b + c of the
//    words g and g + 1 of frame row fa + r, which one v_alignbit by c brings onto bit b; one
//    v_bitop3 ANDs it, or its complement, into the accumulator.  The pattern table is wave-uniform:
//    rows and the set bits of care[r] are walked in scalar registers.  A wave leaves a pattern as
//    soon as its accumulator is zero in every lane.  A lane's anchors are its outer loop and the
//    patterns the inner one (not the other way round): the lane's place in
//    the frame, one integer division, is then computed once per 32 anchors, not once per pattern.
//    Anchors that are none (columns >= width of a replicated torus word, lanes past the last item)
//    start with a zero accumulator bit.  On a plane no anchor needs masking: every pattern has a live
//    cell, and an anchor whose pattern lies wholly outside the rectangle sees only dead cells.
// 3. Counts.  popcount of the match word, wave_sum_dpp's DPP ladder, and lane 63 adds the wave's sum to the
//    pattern's slot in LDS (ds_add_u32; integer sums do not depend on the order).  A slot per
//    pattern instead of per-wave partials behind a barrier per pattern: the waves run through the
//    whole table without meeting.  After the barrier that ends the match, one plain vector store
//    per (board, pattern).  No global atomics: one workgroup owns a board.
// 4. Cover and residue (only with a residue output: a workgroup-uniform run-time switch).  A lane with
//    a nonzero match word ORs, per pattern row, the row's live cells shifted to each of its matching
//    anchors into a cover bitmap of the frame's shape (ds_or_b32 on words g and g + 1).  After the
//    barrier the cover that landed on copies -- margin rows and words, replicas inside a narrow
//    word -- is folded onto the cell it copies, and popcount(board & ~cover) over the real cells is
//    reduced like a count.  Only live cells are ever covered, and outside a plane's rectangle
//    nothing is alive, so the fold needs no topology either.
//
// Barriers.  Three __syncthreads: after the staging, after the match, and (with a residue output)
// after the residue's reduction.  Each sits at the top level of the kernel, outside every loop and
// every branch but `residue != nullptr`, which is a kernel argument: every wave of the workgroup
// reaches each of them exactly once.  The loops between them have trip counts that come from the
// shape, blockDim and the pattern table only; the per-wave early-out of the match (a ballot over the
// wave's accumulators) encloses LDS reads, VALU work and LDS atomics, no barrier.  The wave sum is
// taken where the wave is converged (block sizes are multiples of 64, lanes without an item carry
// zeros instead of leaving the loop).
//
// Bounds.  Frame reads: rows fa + r <= (height + 30) + 31 = FR - 1, words g + 1 <= nw + 1 = FW - 1;
// lanes without an item read item 0.  Board reads: row (height - 1), word nw - 1 <= wd - 1, inside
// the board's pitch.  The launcher refuses shapes the engine cannot have made.
//
// Size.  This header includes golhip_internal.hpp only.  board_common.hpp brings golhip_stencil.hpp,
// whose inline launchers instantiate the four gol_step1 kernels in every translation unit that
// includes it: 15 KB of object for the seven lines of wave_sum_dpp, which the production library's
// size (tests/test_boundary.py) does not have to spare.  So the DPP ladder is written out here.
#pragma once
#include "golhip_internal.hpp"

namespace golhip {
namespace {

constexpr int kCensusMargin = 31;  // pattern rows and columns beyond an anchor, at most

// wave_sum_dpp (golhip_stencil.hpp), the same six steps: the sum of v over the wave's 64 lanes, in
// lane 63 (row_shr 1, 2, 4, 8 inside each 16-lane row, then row_bcast 15 / 31 across the rows).
__device__ __forceinline__ uint32_t census_wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    return v;
}
// acc & (v ^ inv) in one v_bitop3_b32: the truth table indexed by (acc << 2) | (v << 1) | inv
constexpr uint8_t kCensusAndXor = 0xF0 & (0xCC ^ 0xAA);

__global__ __launch_bounds__(1024) void gol_batch_census(const uint32_t *__restrict__ boards, int64_t board_pitch,
                                                         int32_t wd, int32_t width, int32_t height, int32_t plane,
                                                         const CensusPattern *__restrict__ patterns, int32_t npat,
                                                         uint32_t *__restrict__ counts,
                                                         uint32_t *__restrict__ residue) {
    extern __shared__ __attribute__((aligned(16))) uint32_t census_lds[];
    const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x, lane = tid & 63;
    const int H = height;
    const int nw = width >= 32 ? width >> 5 : 1;  // a power of two, as H is
    const int FW = nw + 2, FR = H + 2 * kCensusMargin;
    const uint32_t wmask = width >= 32 ? ~0u : (1u << width) - 1u;
    const bool do_cover = residue != nullptr;
    uint32_t *frame = census_lds, *cnt = frame + FR * FW, *res = cnt + npat, *cover = res + 1;
    const uint32_t *board = boards + (int64_t)blockIdx.x * board_pitch;

    // 1. the frame (and zeros in the cover and the sums); a power of two of lanes per frame row
    {
        const int lg = 32 - __builtin_clz((unsigned)(FW - 1)), j = tid & ((1 << lg) - 1), col = j - 1;
        if (j < FW) {
            for (int fr = tid >> lg; fr < FR; fr += nthreads >> lg) {
                const int y = fr - kCensusMargin;
                uint32_t v = 0;
                if (!plane)
                    v = board[(y & (H - 1)) * wd + (col & (nw - 1))];
                else if (y >= 0 && y < H && col >= 0 && col < nw)
                    v = board[y * wd + col] & wmask;
                frame[fr * FW + j] = v;
                if (do_cover) cover[fr * FW + j] = 0;
            }
        }
        for (int p = tid; p <= npat; p += nthreads) cnt[p] = 0;  // cnt[npat] is *res
    }
    __syncthreads();

    // 2. - 4. the match: anchor rows ay0 .. H + 30 of the frame, word groups ag0 .. nw
    {
        const int ay0 = plane ? 0 : kCensusMargin, ag0 = plane ? 0 : 1;
        const int ng = nw + 1 - ag0, items = (H + kCensusMargin - ay0) * ng;
        for (int base = 0; base < items; base += nthreads) {
            const bool mine = base + tid < items;
            const int idx = mine ? base + tid : 0;
            const int row = idx / ng, g = ag0 + (idx - row * ng), fa = ay0 + row;
            const uint32_t amask = !mine ? 0u : plane ? ~0u : wmask;
            const uint32_t *fp = frame + fa * FW + g;
            uint32_t *cp = cover + fa * FW + g;
            for (int p = 0; p < npat; ++p) {
                const CensusPattern &pt = patterns[p];
                const int ph = pt.h;
                uint32_t acc = amask;
                for (int r = 0; r < ph; ++r) {
                    uint32_t care = pt.care[r];
                    if (care) {
                        const uint32_t alive = pt.alive[r];
                        const uint32_t lo = fp[r * FW], hi = fp[r * FW + 1];
                        do {
                            const int c = __builtin_ctz(care);
                            care &= care - 1;
                            const uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)c);
                            const uint32_t inv = ((alive >> c) & 1u) - 1u;  // a live cell: 0, a dead one: ~0
                            acc = __builtin_amdgcn_bitop3_b32(acc, v, inv, kCensusAndXor);
                        } while (care);
                    }
                    if (__builtin_amdgcn_ballot_w64(acc != 0) == 0) break;  // no lane of the wave can match
                }
                if (__builtin_amdgcn_ballot_w64(acc != 0) == 0) continue;
                const uint32_t n = census_wave_sum((uint32_t)__builtin_popcount(acc));
                if (lane == 63 && counts) atomicAdd(&cnt[p], n);
                if (do_cover && acc) {
                    for (int r = 0; r < ph; ++r) {
                        uint32_t alive = pt.alive[r];
                        if (!alive) continue;
                        uint64_t s = 0;
                        do {
                            const int c = __builtin_ctz(alive);
                            alive &= alive - 1;
                            s |= (uint64_t)acc << c;
                        } while (alive);
                        atomicOr(&cp[r * FW], (uint32_t)s);
                        if ((uint32_t)(s >> 32)) atomicOr(&cp[r * FW + 1], (uint32_t)(s >> 32));
                    }
                }
            }
        }
    }
    __syncthreads();
    if (counts)
        for (int p = tid; p < npat; p += nthreads) counts[(int64_t)blockIdx.x * npat + p] = cnt[p];
    if (!do_cover) return;  // a kernel argument: the whole workgroup leaves, or none of it

    // the fold: every copy of a real word -- the frame rows congruent to its row, the margin word
    // beside the first and the last word, the replicas inside a narrow word -- onto the word
    {
        const int lgnw = 31 - __builtin_clz((unsigned)nw);
        uint32_t n = 0;
        for (int i = tid; i < H * nw; i += nthreads) {
            const int y = i >> lgnw, k = i & (nw - 1);
            uint32_t cov = 0;
            for (int fr = (y + kCensusMargin) & (H - 1); fr < FR; fr += H) {
                cov |= cover[fr * FW + k + 1];
                if (k == nw - 1) cov |= cover[fr * FW];
                if (k == 0) cov |= cover[fr * FW + nw + 1];
            }
            for (int s = 16; s >= width; s >>= 1) cov |= cov >> s;
            n += (uint32_t)__builtin_popcount(frame[(y + kCensusMargin) * FW + k + 1] & wmask & ~cov);
        }
        n = census_wave_sum(n);
        if (lane == 63) atomicAdd(res, n);
    }
    __syncthreads();
    if (tid == 0) residue[blockIdx.x] = *res;
}

// Dynamic LDS of one workgroup: the frame, the cover (with a residue output), the sums.
inline size_t census_lds_bytes(int width, int height, int npat, bool cover) {
    const size_t nw = width >= 32 ? (size_t)width / 32 : 1;
    const size_t fw = (nw + 2) * ((size_t)height + 2 * kCensusMargin);
    return sizeof(uint32_t) * (fw * (cover ? 2 : 1) + (size_t)npat + 1);
}

}  // namespace
}  // namespace golhip
