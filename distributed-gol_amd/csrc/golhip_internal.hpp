// golhip_internal.hpp -- launch-side interface between the engine (golhip_engine.hip) and the
// gfx950 kernels (golhip_kernels.hip).  Not part of the public ABI (include/golhip.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

namespace golhip {

// Two libraries from the same production sources (Makefile):
//   lib/libgolhip.so         production: only the kernels the automatic planner runs (the
//                            production drift stencil at every depth, gol_step1, the production
//                            register-slab shapes); no tuning environment variable is read;
//   lib_tuning/libgolhip.so  the same objects PLUS the tuning-only translation units under
//                            csrc/tuning/: the measured-and-rejected stencil variants, the
//                            level-split and register-tile kernels, the other slab shapes, the
//                            timestamping kernels, the fault-injection hooks and the environment
//                            selectors of the A/B scripts.  Those TUs register themselves in
//                            kernel_extras() (below) / engine_hooks() (golhip_engine.hpp) when the
//                            library loads; the production sources never name the tuning build.

// Device layout of one row strip (see DESIGN.md "Data layout in HBM"):
//   torus width L = lcm(width, 128) bits, wd = L/32 uint32 words per row, LSB-first
//   (bit b of word j is x = 32j+b; identical bytes to LSB-first uint64 words), rows
//   contiguous at `pitch` words; `halo` extra rows above row 0 and below the last row.

// Stencil launch: output rows [r0b, r0e) and [r1b, r1e) (second range may be empty) of the
// strip after K generations, computed from the input strip.
// StencilParams::act layout (uint32 offsets for G slabs): changed[par] at 4 G par (16 bytes per
// slab), same at 8 G, pop at 9 G (16 per slab); kActWords * G in all.
constexpr int kActWords = 25;
__host__ __device__ inline int64_t act_chg_off(int par, int64_t G) { return 4 * G * par; }
__host__ __device__ inline int64_t act_same_off(int64_t G) { return 8 * G; }
__host__ __device__ inline int64_t act_pop_off(int64_t G) { return 9 * G; }
constexpr int kActStatSlots = 64;  // StencilParams::act_stats: [computed x 64][skipped x 64]

// The mixer of init_random_rows (golhip_kernels.hip) and batch_init_random (batch_board.hip): one
// definition, so that a batch's board i is word for word the single engine's board of seed_i.
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// Word `col` (of the torus row's wd words) of row y of the random board of `seed` (width % 64 == 0):
// what init_random_rows and batch_init_random store there, generated straight into registers by
// gol_batch_search (batch_search.hpp).  density 0x80000000 takes 32 bits of one draw per 64 cells,
// every other density compares one draw per cell.  The two init kernels keep the expression in
// their own loops: calling this from batch_init_random changed batch_board.hip's code object
// (another register assignment), and that object is held fixed;
// tests/test_gpu_batch_search.py compares the soups with batch_init_random's boards.
__device__ __forceinline__ uint32_t init_random_word(uint64_t seed, int64_t y, int32_t col, int64_t width,
                                                     uint32_t density) {
    const uint64_t g = 0x9E3779B97F4A7C15ULL;
    const int64_t wpr = width / 64;
    const int64_t x0 = ((int64_t)col * 32) % width;
    uint32_t v = 0;
    if (density == 0x80000000u) {
        const uint64_t wi = (uint64_t)y * wpr + (uint64_t)(x0 >> 6);
        const uint64_t wv = splitmix64(seed + (wi + 1) * g);
        v = (x0 & 32) ? (uint32_t)(wv >> 32) : (uint32_t)wv;
    } else {
        for (int b = 0; b < 32; ++b) {
            const uint64_t cell = (uint64_t)y * width + (uint64_t)(x0 + b);
            const uint32_t d = (uint32_t)splitmix64(seed + (cell + 1) * g);
            v |= (uint32_t)(d < density) << b;
        }
    }
    return v;
}

struct StencilParams {
    int64_t pitch;       // words between consecutive rows
    int64_t r0b, r0e;    // output range 0
    int64_t r1b, r1e;    // output range 1 (r1b == r1e: none)
    int64_t band;        // output rows per wave band
    // > 0: range 0 is nbig0 bands of `band` rows, then bands of band2 rows (shorter: the last
    // dispatched waves are short, so the launch's tail is short -- graded bands)
    int64_t band2, nbig0;
    int64_t nbands0;     // bands in range 0
    int64_t nbands;      // bands in total
    int64_t wrap_rows;   // > 0: single strip holding the whole torus height (row index mod H)
    int64_t lo, hi;      // halo mode: readable input rows [lo, hi) relative to row 0
    int32_t wd;          // words per row of the torus
    int32_t nchunks;     // column chunks per row (chunk_words() words each)
    // 1: the waves raise their issue priority (s_setprio 3) -- the split step's boundary bands,
    // a few dozen waves on the critical path that share SIMDs with the interior's (gol_stencil)
    int32_t prio;
    // nullable: row 0 of a board (same pitch and rows) that receives the XOR of the output
    // generation with the one before it -- the cells the launch's last generation flipped
    // (gol/distributor.go:53-59), written beside the output rows (no extra pass)
    uint32_t *diff;
    // > 0 (gol_slab only; golhip_step_flips): EVERY generation g (0-based) of the launch writes its
    // flips to diff + g * diff_stride words (consecutive slots of the per-turn flips ring)
    int64_t diff_stride;
    // null in production; the tuning library's stamp handles: gol_slab2's per-wave phase stamps,
    // 8 uint64 per wave (golhip_tuning_stamps_ex, scripts/slab_stamps.py)
    uint64_t *stamp;
    // Stable-slab skipping (gol_slab2 ACT, single-strip torus boards; null: off).  act holds, per slab
    // (workgroup) g of G = nbands * nchunks (offsets: act_*_off below, kActWords * G uint32 in all):
    // changed[2] -- 16 bytes per slab, byte w: did wave w's output rows change in the last generation
    // of the launch that wrote them (this launch reads changed[act_par], writes changed[act_par ^ 1]);
    // same -- both ping-pong buffers hold the slab's output region identically; pop -- 16 uint32
    // per slab, wave w's alive cells at that last generation.  Per-wave entries written with plain
    // stores: one shared flag per slab took an OR / add atomic from every wave (+11 % kernel time on
    // dense boards, profiles/r05/r05n_act_ablation.log).  act_reset: the flags are stale (a new
    // board, another kernel or slab shape ran): every slab computes and rewrites them.
    // act_stats (nullable): slabs computed / skipped, spread over kActStatSlots uint64 each (slot
    // group % kActStatSlots: one shared counter serialised ~10 ns per workgroup at L2).
    uint32_t *act;
    unsigned long long *act_stats;
    int32_t act_par, act_reset;
};

constexpr int kMaxK = 32;         // generations per launch limit (halo lane = 32 bits)
constexpr int kCountSlots = 64;   // per-generation count slots (spread the atomics)

// Stencil variants: levels of a step as one dependent chain or skewed across steps (K-way ILP),
// with 1 or 2 words (32 / 64 cells) per lane.
constexpr int kVariantSkew = 0;
constexpr int kVariantChain = 1;
constexpr int kVariantSkewD2 = 2;
constexpr int kVariantChainD2 = 3;
constexpr int kVariantSkewLdsPf = 4;   // input rows prefetched by LDS-DMA instead of VGPRs
constexpr int kVariantChainLdsPf = 5;
constexpr int kVariantSkewLdsD2 = 6;   // LDS-DMA ring, 2 words (64 cells) per lane
constexpr int kVariantChainLdsD2 = 7;
constexpr int kVariantDriftLds = 8;    // chained LDS-DMA levels with drifting row sums (K <= 16)
constexpr int kVariantDriftZip = 9;    // drift, 62-word chunks, two steps interleaved (ZIP = 2)
constexpr int kVariantDrift62 = 10;    // drift, 62-word chunks (one whole-word store per step)
constexpr int kVariantDriftNoFill = 11;  // driftlds without the compile-time unrolled fill
// Production: drifting sums at every depth, with the chunk geometry measured fastest per depth:
// at K = 16 the pre-shifted 63-word rows (PRE, below; round 3: +2.9 % at 65536^2 and +3.0 % at
// 262144^2 over the half-word halo, pre-heated lockstep A/B, profiles/r03/r03p_ab_*.log), 62-word
// chunks (one store per step) at every other K >= 2 (PRE measured equal at K = 12, +0.6 % at 8;
// profiles/r02/tune_depth_geometry.txt for the earlier geometries); gol_step1 at K = 1.
constexpr int kVariantProd = 12;
// drift with the input rows pre-shifted K bits west (gol_stencil PRE): 63-word chunks, one whole-word
// store per step, no store realignment (K <= 16; drift62 above)
constexpr int kVariantPre63 = 13;
// production with the lanes of the last column chunk that nothing depends on exec-masked off
constexpr int kVariantProdMask = 14;
// production with per-wave timestamps (tuning build: dispatch skew, wave durations, per-SIMD
// tails and the in-kernel clock of a launch; golhip_tuning_stamps)
constexpr int kVariantStamp = 15;
constexpr int kNumVariants = 16;
// The pre-shifted geometry in production: every non-counting launch of depth 2..16 (the driver's
// dense 20-turn region, pre-heated: +1.2 % over the 62-word chunks, profiles/r03/r03aa_ab_split.log;
// K = 16 +2.9 %), and counting launches at K = 16 only (with counts at K < 16 its allocator holds
// 168 VGPRs, 3 waves per SIMD, against the 62-word kernel's 110 and 4).
constexpr bool prod_pre(int K, bool counting = false) { return K == 16 || (!counting && K >= 2 && K < 16); }
// Variants of the production family: gol_step1 at K = 1, the level-split kernel for small boards.
inline bool variant_is_production_family(int v) {
    return v == kVariantChainLdsPf || v == kVariantDriftLds || v == kVariantDriftZip ||
           v == kVariantDrift62 || v == kVariantDriftNoFill || v == kVariantProd || v == kVariantPre63 ||
           v == kVariantProdMask || v == kVariantStamp;
}
inline int variant_words(int v) {
    return (v == kVariantSkewD2 || v == kVariantChainD2 || v == kVariantSkewLdsD2 ||
            v == kVariantChainLdsD2)
               ? 2
               : 1;
}
// Words of a row owned by one wave of the stencil (its column chunk): 62 lanes x D words, or 63
// words with the half-word halo (D = 1, K <= 16: lanes 0 and 63 own half a word each).
constexpr int kStep1WavesPerCu = 8;  // gol_step1 grid: resident waves per CU it is sized for
inline int chunk_words(int K, int variant, bool counting = false) {
    if (K == 1 && variant_is_production_family(variant))
        return 256;  // gol_step1: 4 words x 64 lanes
    const int d = variant_words(variant);
    if (variant == kVariantDriftZip || variant == kVariantDrift62) return 62;
    if (variant == kVariantProd || variant == kVariantProdMask || variant == kVariantStamp)
        return prod_pre(K, counting) ? 63 : 62;
    if (variant == kVariantPre63) return K <= 16 ? 63 : 62;
    return (d == 1 && K <= 16) ? 63 : 62 * d;
}

// Production launch depths, one translation unit each (stencil_k<K>.hip).  The tuning library adds
// K = 20 / 24 through kernel_extras().
#define GOLHIP_STENCIL_DEPTHS(X) X(1) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(32)
#define GOLHIP_X(K)                                                                           \
    hipError_t launch_stencil_k##K(const uint32_t *in, uint32_t *out, const StencilParams &p, \
                                   unsigned long long *slots, hipStream_t s);                \
    const void *stencil_fn_k##K();                                                            \
    hipError_t warm_stencil_k##K(hipStream_t s);
GOLHIP_STENCIL_DEPTHS(GOLHIP_X)
#undef GOLHIP_X

// ---- life-like rules (gol_rule, golhip_rule.hpp; one translation unit per depth, rule_k<K>.hip) ----
// Outer-totalistic rules on the Moore neighbourhood as two 9-bit masks: birth bit n = a dead cell
// with n live neighbours is born, survive bit n = a live cell with n live neighbours stays alive.
// B3/S23 runs the production kernels above; every other rule runs gol_rule (launch kind 5).
constexpr uint32_t kRuleMaskBits = 0x1ffu;
constexpr uint32_t kLifeBirth = 0x008u, kLifeSurvive = 0x00Cu;
struct RuleMasks {
    uint32_t birth, survive;
};
// Rules with a constant-folded instantiation (RuleConst<B, S>: the rule's truth tables are v_bitop3
// immediates); every other rule runs the table form (RuleTable: the 18 rule bits are kernel
// arguments).  One entry per rule: X(birth mask, survive mask).
#define GOLHIP_RULE_CATALOGUE(X)                    \
    X(0x048, 0x00C) /* HighLife     B36/S23      */ \
    X(0x1C8, 0x1D8) /* Day & Night  B3678/S34678 */ \
    X(0x004, 0x000) /* Seeds        B2/S         */ \
    X(0x0AA, 0x0AA) /* Replicator   B1357/S1357  */
inline bool rule_catalogued(uint32_t birth, uint32_t survive) {
#define GOLHIP_X(B, S) \
    if (birth == (B) && survive == (S)) return true;
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return false;
}
// Launch depths of gol_rule: any turn count decomposes; the rule path runs the largest depth that
// fits (rule_pick_k).
#define GOLHIP_RULE_DEPTHS(X) X(1) X(2) X(4) X(8)
constexpr int kRuleChunkWords = 62;  // lanes 1..62 store whole words (drifting sums, K <= 32)
inline int rule_pick_k(int64_t n) { return n >= 8 ? 8 : n >= 4 ? 4 : n >= 2 ? 2 : 1; }
#define GOLHIP_X(K)                                                                            \
    hipError_t launch_rule_k##K(RuleMasks rm, const uint32_t *in, uint32_t *out,              \
                                const StencilParams &p, unsigned long long *slots, hipStream_t s); \
    const void *rule_fn_k##K(RuleMasks rm, bool counting);
GOLHIP_RULE_DEPTHS(GOLHIP_X)
#undef GOLHIP_X
// Launch the K-generation rule stencil (K one of GOLHIP_RULE_DEPTHS), same StencilParams contract
// as launch_stencil (both ranges, graded bands, wrap / halo rows, prio, slots, diff).
hipError_t launch_rule(int K, RuleMasks rm, const uint32_t *in_row0, uint32_t *out_row0,
                       const StencilParams &p, unsigned long long *count_slots, hipStream_t s);
// Resident waves per CU of this rule's K-deep launch (occupancy query), for sizing the grid.
int rule_waves_per_cu(int K, RuleMasks rm, bool counting);

// Kernels beyond the production set.  Empty in the production library; the tuning library's
// TUs (csrc/tuning/) fill it from static initialisers when the library loads.  Every dispatcher
// asks the production kernels first and falls back to an entry here (a null entry: the kernel is
// not in this library).
using StencilLaunchFn = hipError_t (*)(int variant, const uint32_t *in, uint32_t *out,
                                       const StencilParams &p, unsigned long long *slots,
                                       hipStream_t s);
struct KernelExtras {
    // per depth: every kernel variant of that depth (the tuning variants, and the depths
    // production lacks: K = 20 / 24); fn / warm as stencil_fn_k / warm_stencil_k
    StencilLaunchFn stencil[kMaxK + 1] = {};
    const void *(*stencil_fn[kMaxK + 1])(int variant) = {};
    hipError_t (*stencil_warm[kMaxK + 1])(int variant, hipStream_t s) = {};
    // gol_step1 configurations other than the production one (GOLHIP_STEP1); null: production
    hipError_t (*step1)(const uint32_t *in, uint32_t *out, const StencilParams &p,
                        unsigned long long *slots, hipStream_t s) = nullptr;
    const void *(*step1_fn)() = nullptr;
    // the level-split kernel, the register tiles, the slab shapes and slab variants production
    // lacks
    bool (*split_supported)(int K, int S) = nullptr;
    hipError_t (*split)(int K, int S, const uint32_t *in, uint32_t *out, const StencilParams &p,
                        unsigned long long *slots, hipStream_t s) = nullptr;
    hipError_t (*split_warm)(hipStream_t s) = nullptr;
    bool (*tile_supported)(int K, int T) = nullptr;
    hipError_t (*tile)(int K, int T, const uint32_t *in, uint32_t *out, const StencilParams &p,
                       unsigned long long *slots, hipStream_t s) = nullptr;
    bool (*slab_supported)(int K, int W, int S, int NC) = nullptr;
    // also every slab launch with p.stamp set (the timestamping slab kernels)
    hipError_t (*slab)(int K, int W, int S, int NC, const uint32_t *in, uint32_t *out,
                       const StencilParams &p, unsigned long long *slots, hipStream_t s) = nullptr;
    // bytes of unused dynamic LDS per stencil block (GOLHIP_LDS_PAD: caps resident blocks per CU)
    size_t lds_pad = 0;
};
KernelExtras &kernel_extras();

// Unused dynamic LDS per stencil block: 0 in production.
inline size_t lds_pad_bytes() { return kernel_extras().lds_pad; }

// Launch the K-generation stencil (a production depth, or one kernel_extras() adds). count_slots (nullable) receives
// per-generation alive counts in kCountSlots slots per generation.
hipError_t launch_stencil(int K, int variant, const uint32_t *in_row0, uint32_t *out_row0,
                          const StencilParams &p, unsigned long long *count_slots,
                          hipStream_t s);
bool stencil_k_supported(int K);
// Load every stencil code object (one per depth TU + the level-split TU) with empty launches, so
// no code-object load lands inside a timed or latency-sensitive step.
hipError_t warm_stencils(int variant, hipStream_t s);
hipError_t warm_stencil_split(hipStream_t s);
// Level-split stencil (small boards): the K levels of a (band, chunk) over a workgroup of S waves
// (S = 2 or 4, D = 1, LDS-DMA input, chained levels; same geometry as kVariantChainLdsPf).
hipError_t launch_stencil_split(int K, int S, const uint32_t *in_row0, uint32_t *out_row0,
                                const StencilParams &p, unsigned long long *count_slots,
                                hipStream_t s);
bool stencil_split_supported(int K, int S);
// Register-tile stencil (small boards, stencil_tile.hip): each wave holds T + 2K rows of a 62-word
// column chunk in VGPRs and runs the K generations over them in place; T output rows per wave.
hipError_t launch_stencil_tile(int K, int T, const uint32_t *in_row0, uint32_t *out_row0,
                               const StencilParams &p, unsigned long long *count_slots,
                               hipStream_t s);
bool stencil_tile_supported(int K, int T);
// Register slab (stencil_tile.hip): a workgroup of W waves, S rows each, edge rows swapped through
// LDS every generation; T = W*S - 2K output rows per workgroup.
// NC: independent row chains per wave (segments advanced op-major).
hipError_t launch_stencil_slab(int K, int W, int S, int NC, const uint32_t *in_row0, uint32_t *out_row0,
                               const StencilParams &p, unsigned long long *count_slots,
                               hipStream_t s);
bool stencil_slab_supported(int K, int W, int S, int NC = 4);
// the slab shapes that can write EVERY generation's flips (StencilParams::diff_stride > 0): the
// production shapes pick_reg_kernel chooses
bool stencil_slab_flips_every_gen(int K, int W, int S, int NC = 4);
// the slab shapes whose launches can skip stable slabs (StencilParams::act): the production gol_slab2
// shapes, without flips
bool stencil_slab_activity(int K, int W, int S, int NC);
hipError_t warm_stencil_tile(hipStream_t s);
// The whole-board kernel (stencil_board.hip): one workgroup holds a board of wd in {4, 8, 16} words
// and `height` = 4 W R rows in registers and runs K (runtime, <= kBoardMaxK) generations in one
// launch.  stencil_board_shape: whether the board fits, and its (W waves, R rows per segment).
constexpr int kBoardMaxK = 4096;
// Automatic use (golhip_set_board_kernel -1): boards of at most this many rows.  One CU issues the
// whole board's VALU work per generation, so the kernel gains while the board is short and loses
// beyond: us per turn, board / slab kernels, calls of 1000 turns with counts
// (profiles/r05/r05k_board_ab.log): 16^2 0.31 / 0.52, 64^2 0.37 / 0.53, 128^2 0.42 / 0.53,
// 256^2 0.57 / 0.54, 512^2 0.88 / 0.55.
constexpr int64_t kBoardAutoRows = 256;
bool stencil_board_shape(int64_t height, int32_t wd, int *W, int *R);
hipError_t launch_stencil_board(int K, int W, int R, const uint32_t *in_row0, uint32_t *out_row0,
                                const StencilParams &p, unsigned long long *slots, hipStream_t s);
// The batch kernel (batch_board.hip): nboards independent tori of that geometry, one workgroup
// each, advanced K generations IN PLACE.  Board i is rows x wd words at boards + i * board_pitch.
struct BatchParams {
    uint32_t *boards;
    int64_t board_pitch;  // words between boards: 4 W R wd
    int32_t wd;           // words per torus row: 4, 8 or 16
    int32_t width;        // cells per board row (counts take one copy of a replicated row)
    // nullable: hist[i * K + g] = alive cells of board i after generation g of the launch
    uint32_t *hist;
    // settle tracking (both or neither): prev holds board(t0 - 1) of every board in the boards'
    // layout (read unless t0 == 0, rewritten with board(t0 + K - 1)); last_diff[i] is raised to the
    // last absolute turn t in (t0, t0 + K] with board_i(t) != board_i(t - 2)
    uint32_t *prev;
    unsigned long long *last_diff;
    int64_t t0;  // turns completed before the launch
};
hipError_t launch_batch_board(int K, int W, int R, int nboards, const BatchParams &p, hipStream_t s);
// The batch kernel for life-like rules (gol_batch_rule, batch_rule.hpp; one translation unit per
// functor, batch_rule_*.hip): gol_batch's contract (b) under `rule`, or, with rules != null, board i
// under its own pair rules[2 i] = birth, rules[2 i + 1] = survive (device memory, nboards pairs).
// A uniform catalogue rule runs its constant-folded kernel; every other uniform rule and every
// launch with per-board rules runs the table form.  B3/S23 as a uniform rule is launch_batch_board's.
struct BatchRuleParams {
    BatchParams b;
    RuleMasks rule;
    const uint32_t *rules;
};
hipError_t launch_batch_rule(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s);
#define GOLHIP_X(B, S)                                                                                    \
    hipError_t launch_batch_rule_##B##_##S(int K, int W, int R, int nboards, const BatchRuleParams &rp, \
                                           hipStream_t s);
GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
// The batch kernel with per-board cycle detection (gol_batch_period, batch_period.hpp; one
// translation unit per functor, batch_period_*.hip): gol_batch's contract (b, without prev /
// last_diff) under `rule` or, with rules != null, per-board rules as in BatchRuleParams -- B3/S23
// included, which runs gol_batch's rule step.  snap (the layout of boards) holds every board's
// Brent snapshot board(2^j - 1), repeat_turn[i] the first turn at which board i equalled its
// snapshot (-1: none yet); both live across launches, b.t0 carries the turn.
struct BatchPeriodParams {
    BatchParams b;
    RuleMasks rule;
    const uint32_t *rules;
    uint32_t *snap;
    int64_t *repeat_turn;
};
hipError_t launch_batch_period(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s);
hipError_t launch_batch_period_life(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s);
#define GOLHIP_X(B, S)                                                                                        \
    hipError_t launch_batch_period_##B##_##S(int K, int W, int R, int nboards, const BatchPeriodParams &pp, \
                                             hipStream_t s);
GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
// The soup search (gol_batch_search, batch_search.hpp; one translation unit per functor,
// batch_search_*.hip): workgroup i generates the board of seed_i = seeds ? seeds[i] : seed0 + i in
// registers (init_random_word), runs it from generation 0 under `rule` -- or, with rules != null,
// under its own pair -- with gol_batch_period's cycle detection until it repeats or max_turns have
// run, and writes out[i].  No board memory: a soup's footprint is its record.
struct SoupRecord {  // golhip_soup_t (include/golhip.h)
    int64_t repeat_turn, period, stop_turn;
    uint32_t population, reserved;
};
constexpr int64_t kSearchMaxTurns = 1 << 20;
struct BatchSearchParams {
    const uint64_t *seeds;  // device memory, one per soup of the launch, or null
    uint64_t seed0;
    uint32_t density;  // q32
    int32_t wd;        // words per torus row: 4, 8 or 16
    int32_t width;     // cells per board row, a multiple of 64
    int32_t max_turns;
    RuleMasks rule;
    const uint32_t *rules;  // device memory, one (birth, survive) pair per soup, or null
    SoupRecord *out;
};
hipError_t launch_batch_search(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s);
hipError_t launch_batch_search_life(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s);
#define GOLHIP_X(B, S) \
    hipError_t launch_batch_search_##B##_##S(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s);
GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
// The batch kernels on a bounded plane (batch_plane.hpp; translation units batch_plane_*.hip): the
// contracts of launch_batch_rule (uniform B3/S23 included, which runs gol_batch's rule step),
// launch_batch_period and launch_batch_search with every neighbour outside the width x height
// rectangle dead.  Two functors: B3/S23's rule step for a uniform B3/S23, the table form for every
// other rule and for per-board rules.  The torus launches above never reach these.
hipError_t launch_plane_rule(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s);
hipError_t launch_plane_rule_life(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s);
hipError_t launch_plane_period(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s);
hipError_t launch_plane_period_life(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s);
// The soup box: cells outside columns [x0, x0 + w) and rows [y0, y0 + h) of a soup are cleared.
struct SoupBox {
    int32_t x0, y0, w, h;
};
// The bits of word `col` (of wd words) of row y whose cells lie in the box; width % 32 == 0.
__device__ __forceinline__ uint32_t box_word_mask(int64_t y, int32_t col, int32_t width, const SoupBox &bx) {
    if (y < bx.y0 || y >= (int64_t)bx.y0 + bx.h) return 0u;
    const int32_t x0 = (col * 32) % width;
    const int32_t lo = min(max(bx.x0 - x0, 0), 32), hi = min(max(bx.x0 + bx.w - x0, 0), 32);
    if (hi <= lo) return 0u;
    const uint32_t below_hi = hi == 32 ? ~0u : (1u << hi) - 1u;
    return below_hi & ~((1u << lo) - 1u);  // lo < hi <= 32
}
// A search on the plane, or a boxed search on either topology (plane == 0: the torus, which only a
// box brings here): BatchSearchParams with the box (the whole board: no box) applied at seeding.
struct BatchBoxSearchParams {
    BatchSearchParams s;
    SoupBox box;
    int32_t plane;
};
hipError_t launch_plane_search(int W, int R, int nsoups, const BatchBoxSearchParams &bp, hipStream_t s);
hipError_t launch_plane_search_life(int W, int R, int nsoups, const BatchBoxSearchParams &bp, hipStream_t s);
// The exact pass of golhip_batch_search_exact (gol_batch_cycle, batch_cycle.hpp; translation units
// batch_cycle_life.hip and batch_cycle_table.hip).  It runs after launch_batch_search or
// launch_plane_search on the same chunk with the same parameters (bp.box the whole board and
// bp.plane 0 for an unboxed torus), reads soup i's (repeat_turn, period) from bp.s.out[i] and writes
// cycle_start[i]: the least t >= 0 with board(t + period) == board(t), -1 without a repeat.  Two
// functors: B3/S23's rule step for a uniform B3/S23, the table form for everything else;
// launch_batch_cycle (engine_batch.hip) checks the parameters and picks one.
// With ash set (golhip_batch_search_census) the pass also hands over a board on each soup's cycle:
// soup i's at ash + i * board_pitch in the batch layout (board_pitch = height * wd words, one copy
// of each replicated row as the step kernels store it), and ash_turn[i] = the turn of that board:
// cycle_start <= ash_turn <= repeat_turn; 0 with the seeded board for a soup that is on its cycle at
// turn 0; -1, and no row written, for a soup without a repeat (the caller zeroes the buffer first).
// With ash null the pass writes cycle_start only, as it always did, and ash_turn is not looked at.
struct BatchCycleParams {
    BatchBoxSearchParams bp;
    int64_t *cycle_start;  // device memory, one per soup of the launch
    uint32_t *ash;         // device memory, nsoups boards, or null
    int64_t *ash_turn;     // device memory, one per soup of the launch; written whenever ash is set
};
hipError_t launch_batch_cycle(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s);
hipError_t launch_batch_cycle_life(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s);
hipError_t launch_batch_cycle_table(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s);
// The census (gol_batch_census, batch_census.hpp; ONE kernel in one translation unit, batch_census.hip,
// with run-time width, height, topology and pattern table): board i of the launch is boards + i *
// board_pitch in the batch layout, nboards <= 65536.  counts[i * npat + p] = the anchors at which
// pattern p matches board i, residue[i] = the live cells of board i that no match covers
// (include/golhip.h: golhip_batch_census); either may be null, not both.  A null residue skips the
// cover work.  All pointers are device memory.
struct CensusPattern {  // golhip_pattern_t (include/golhip.h)
    int32_t w, h;
    uint32_t alive[32], care[32];
};
constexpr int kCensusMaxPatterns = 256;
struct BatchCensusParams {
    const uint32_t *boards;
    int64_t board_pitch;
    int32_t wd, width, height;  // words per torus row, cells per board row, rows
    int32_t plane;
    const CensusPattern *patterns;
    int32_t npat;  // 1 .. kCensusMaxPatterns
    uint32_t *counts, *residue;
};
hipError_t launch_batch_census(int nboards, const BatchCensusParams &cp, hipStream_t s);
// The objects (gol_batch_objects, batch_objects.hpp; ONE kernel in one translation unit,
// batch_objects.hip, with run-time width, height, topology, reach and cap): board i of the launch is
// boards + i * board_pitch in the batch layout, nboards <= 65536.  nobjects[i] = the clusters of
// board i, all of them; objects, if set, holds `window` records per board, and cluster j of board i
// (include/golhip.h: golhip_batch_objects has the definitions and the order) is stored at
// objects[i * window + j - first] when first <= j < min(first + window, max_objects).  All pointers
// are device memory.
struct ObjectRecord {  // golhip_object_t (include/golhip.h)
    int32_t x, y, w, h;
    int32_t population;
    uint32_t flags;
    uint64_t hash;
};
constexpr int kObjectsMax = 4096;
constexpr uint32_t kObjectWindsX = 1u, kObjectWindsY = 2u, kObjectAtBorder = 4u;
struct BatchObjectsParams {
    const uint32_t *boards;
    int64_t board_pitch;
    int32_t wd, width, height;  // words per torus row, cells per board row, rows
    int32_t plane;
    int32_t reach;        // 1 or 2
    int32_t max_objects;  // 1 .. kObjectsMax
    int32_t first, window;
    int32_t *nobjects;
    ObjectRecord *objects;  // or null: the counts alone
};
hipError_t launch_batch_objects(int nboards, const BatchObjectsParams &op, hipStream_t s);
// Clears every cell outside the box in boards of the batch layout (after launch_batch_init_random).
hipError_t launch_batch_clip_box(uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows, int64_t width,
                                 int32_t wd, const SoupBox &box, hipStream_t s);
// init_random_rows for every board: board i from seeds ? seeds[i] (device memory) : seed0 + i.
hipError_t launch_batch_init_random(uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                                    int64_t width, int32_t wd, const uint64_t *seeds, uint64_t seed0,
                                    uint32_t density_q32, hipStream_t s);
// out[i] = alive cells of board i.
hipError_t launch_batch_popcount(const uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                                 int64_t width, int32_t wd, uint32_t *out, hipStream_t s);
constexpr int kTileChunkWords = 62;
// Words per column chunk of the level-split kernel (half-word halo for K <= 16).
__host__ __device__ constexpr int split_chunk_words(int K) { return K <= 16 ? 63 : 62; }
// Resident waves per CU of the stencil launch (occupancy query), for sizing the grid.
int stencil_waves_per_cu(int K, int variant);
// Sum the slots of K generations into counts[0..K) and zero the slots.
hipError_t launch_count_finalize(int K, unsigned long long *slots, unsigned long long *counts,
                                 hipStream_t s);

// 0/nonzero bytes (rows x width, compact, stride == width) -> packed torus rows.
hipError_t launch_pack(const uint8_t *bytes, int64_t rows, int64_t width, int32_t wd,
                       uint32_t *row0, int64_t pitch, hipStream_t s);
// First `width` columns of packed rows -> 0/255 bytes (compact, stride == width).
hipError_t launch_unpack(const uint32_t *row0, int64_t pitch, int64_t rows, int64_t width,
                         uint8_t *bytes, hipStream_t s);
// Counter-based random rows; gy0 = global index of local row 0.
hipError_t launch_init_random(uint32_t *row0, int64_t pitch, int64_t rows, int64_t gy0,
                              int64_t width, int32_t wd, uint64_t seed, uint32_t density_q32,
                              hipStream_t s);
// Popcount of rows x wd words, added into *out.
hipError_t launch_popcount(const uint32_t *row0, int64_t pitch, int64_t rows, int32_t wd,
                           unsigned long long *out, hipStream_t s);
// Alive-cell / flip extraction (row-major): cells are bits of (a ^ b) (b nullable) in the first
// `width` columns.  row_counts[rows], offsets[rows+1], block_sums[kScanBlocks] are scratch;
// offsets = the exclusive scan of the row counts, offsets[rows] = total.  Multi-block: every
// block counts a contiguous range of rows, one block scans the block sums, every block then scans
// its range (three launches, no serial walk over the rows).
constexpr int kScanBlocks = 1024;
hipError_t launch_extract_count(const uint32_t *a, const uint32_t *b, int64_t pitch,
                                int64_t rows, int64_t width, uint32_t *row_counts,
                                unsigned long long *offsets, unsigned long long *block_sums,
                                hipStream_t s);
// slot_rows: rows per slot of a tall board of slots (y is reported within its slot).
hipError_t launch_extract_emit(const uint32_t *a, const uint32_t *b, int64_t pitch,
                               int64_t rows, int64_t width, const unsigned long long *offsets,
                               int64_t gy0, int64_t slot_rows, int32_t *xy, uint64_t cap,
                               hipStream_t s);
// x coordinates only, as uint16 (width <= 65536), in the same order (golhip_step_flips_rows).
hipError_t launch_extract_emit_x16(const uint32_t *a, const uint32_t *b, int64_t pitch,
                                   int64_t rows, int64_t width, const unsigned long long *offsets,
                                   uint16_t *x, uint64_t cap, hipStream_t s);
// counts[t] = cells of slot t (rows [t * slot_rows, (t+1) * slot_rows)) from the extract scan.
hipError_t launch_extract_slot_counts(const unsigned long long *offsets, int64_t slot_rows,
                                      int64_t slots, unsigned long long *counts, hipStream_t s);
// Packed torus rows <-> logical uint64 words (width % 64 == 0; first width bits of each row).
hipError_t launch_words_out(const uint32_t *row0, int64_t pitch, int64_t rows, int64_t width,
                            uint64_t *words, hipStream_t s);
hipError_t launch_words_in(const uint64_t *words, int64_t rows, int64_t width, int32_t wd,
                           uint32_t *row0, int64_t pitch, hipStream_t s);

// ---- windowed access (view_kernels.hip) --------------------------------------------------------
// x0 is a logical column in [0, width); columns past it are taken mod the torus (wd words).
// The density viewport: out[jj * w + i] = live cells of the scale x scale block whose columns are
// x0 + i * scale onward and whose rows are rows [jj * scale - phase, + scale) of the `nrows` rows at
// rows0, clipped to them (a pixel row cut by the end of a strip gives a partial count); npr pixel
// rows, scale a power of two in 1..1024, phase < scale.
hipError_t launch_view_counts(const uint32_t *rows0, int64_t pitch, int64_t nrows, int32_t phase, int32_t wd,
                              int64_t x0, int32_t scale, int32_t w, int64_t npr, uint32_t *out, hipStream_t s);
// Columns [x0, x0 + w) of packed rows -> 0/255 bytes (compact, stride == w).
hipError_t launch_rect_unpack(const uint32_t *row0, int64_t pitch, int64_t rows, int32_t wd, int64_t x0,
                              int64_t w, uint8_t *bytes, hipStream_t s);
// 0/nonzero bytes (compact, stride == w) into columns [x0, x0 + w) of packed rows, in every
// horizontal replica of the torus: mode 0 copy, 1 or, 2 xor (a masked read-modify-write).
hipError_t launch_rect_pack(const uint8_t *bytes, int64_t rows, int64_t width, int32_t wd, int64_t x0, int64_t w,
                            int mode, uint32_t *row0, int64_t pitch, hipStream_t s);

}  // namespace golhip
