// engine_batch.hip -- golhip_batch: many independent small tori on one device, a second handle
// type beside the engine (golhip_engine.hip).
//
// The reference runs one world per broker (broker/broker.go:157-180); a soup search, a seed or
// density sweep or a census runs thousands of small ones.  A batch holds nboards tori of one size
// -- the sizes of the whole-board kernel, stencil_board_shape: 4, 8 or 16 torus words wide, 4 W R
// rows -- back to back in one allocation, board i at boards + i * height * wd words in the packed
// layout of a single engine of that size, and advances all of them with one gol_batch launch per
// <= kBoardMaxK generations (batch_board.hip: one workgroup per board, in place).
//
// The rule.  A batch starts at B3/S23 and a uniform B3/S23 always launches gol_batch.  Any other
// life-like rule -- one for all boards (golhip_batch_set_rule / _set_rule_masks) or one per board
// (golhip_batch_set_rules) -- launches gol_batch_rule (batch_rule.hpp): constant-folded for a
// uniform catalogue rule, the table form for every other uniform rule and for per-board rules
// whatever they are.  golhip_batch_kernel reports which.  The settle record is the record of one
// rule, so with tracking on the rule changes at turn 0 only.
//
// Period tracking (golhip_batch_track_period) swaps every one of those launches for gol_batch_period
// (batch_period.hpp) under the same rule: per-board Brent cycle detection, a snapshot buffer beside
// the boards and one int64 per board.  golhip_batch_kernel's form still names the rule form.  It
// excludes settle tracking (one tracker per launch keeps the kernel count down), and its record
// too is the record of one rule.
//
// The soup search (golhip_batch_search) runs gol_batch_search (batch_search.hpp): soups are seeds, not
// boards of the batch.  The handle lends its size, device, stream and uniform rule; its boards, turn,
// records and switches are not touched.  Soups go out in chunks of at most kSearchChunk soups and
// at most 2^44 cell updates, so that no launch runs long on a shared device.
// golhip_batch_search_exact is the same call with a second pass per chunk, gol_batch_cycle
// (batch_cycle.hpp), which turns each record's (repeat_turn, period) into the soup's cycle_start, the
// first turn of its cycle; launch_batch_cycle below picks its functor.  golhip_batch_search_census is
// the exact call whose pass also stores, per soup, a board on the soup's cycle into a chunk-sized
// ash buffer (at most 64 MiB, allocated by the first such call), over which the census runs:
// search_run has the order of a chunk.
//
// Device memory is allocated at create (the boards, the per-board counters, the transfer stage), by
// the first golhip_batch_track_settle(b, 1) (board(t - 1) of every board), by the first
// golhip_batch_track_period(b, 1) (every board's snapshot and its repeat turn) and by the first
// golhip_batch_set_rules (the per-board rule pairs) and by the first golhip_batch_search or
// golhip_batch_search_exact (one chunk's seeds, rule pairs, records and cycle starts) and by the first
// golhip_batch_census (the pattern table, 66 KiB); no other call allocates.  Bytes in and out,
// the seeds of init_random, per-board rules and counts, the per-turn history and the census's counts
// and residues all pass through the stage in chunks.
//
// The census (golhip_batch_census) runs gol_batch_census (batch_census.hpp) over the boards as they are:
// it reads the boards and the topology and writes nothing the handle owns.
//
// The objects (golhip_batch_objects) run gol_batch_objects (batch_objects.hpp) over the boards in the same
// way, and golhip_batch_search_objects runs it over a chunk's ash where the search census runs the census.
// Their counts and records come back through the search census's stage and, the records, through
// pinned host memory, both allocated by the first call that needs them: objects_boards.
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "golhip_engine.hpp"

struct golhip_batch {
    int64_t width = 0, height = 0, L = 0;
    int32_t wd = 0;
    int W = 0, R = 0;  // the kernel's shape: 4 W R == height
    int nboards = 0, device = 0;
    int64_t board_words = 0;  // height * wd
    hipStream_t stream = nullptr;
    uint32_t *boards = nullptr;
    uint32_t *prev = nullptr;                 // settle tracking: board(turn - 1) of every board
    unsigned long long *last_diff = nullptr;  // last turn t with board(t) != board(t - 2); 0: none yet
    uint8_t *stage = nullptr;
    int64_t stage_bytes = 0;
    bool track = false;
    uint32_t *snap = nullptr;        // period tracking: board(2^j - 1) of every board, the Brent snapshot
    int64_t *repeat_turn = nullptr;  // first turn t with board(t) == board(s(t)); -1: none yet
    bool track_period = false;
    int64_t turn = 0;
    golhip::RuleMasks rule{golhip::kLifeBirth, golhip::kLifeSurvive};  // the uniform rule
    bool per_board = false;              // the boards run `rules`, not `rule`
    uint32_t *rules = nullptr;           // device: nboards (birth, survive) pairs
    std::vector<uint32_t> rules_host;    // the same pairs, for golhip_batch_get_rules
    // golhip_batch_search / _search_exact: one chunk's seeds, rule pairs and records
    uint64_t *search_seeds = nullptr;
    uint32_t *search_rules = nullptr;
    golhip::SoupRecord *search_out = nullptr;
    int64_t *search_cycle = nullptr;  // golhip_batch_search_exact: the chunk's cycle starts
    uint32_t *search_ash = nullptr;       // golhip_batch_search_census: one chunk's boards, at most 64 MiB
    int64_t *search_ash_turn = nullptr;   // and their turns
    uint8_t *search_stage = nullptr;      // and the stage their census and cells come back through
    int64_t search_stage_bytes = 0;
    int64_t stage_limit = 0;              // GOLHIP_STAGE_BYTES at create, 0 without: it caps that stage too
    golhip::CensusPattern *census_pat = nullptr;  // golhip_batch_census: the pattern table of a call
    uint8_t *objects_host = nullptr;      // golhip_batch_objects / _search_objects: a chunk's records on the
    int64_t objects_host_bytes = 0;       // host (pinned), from which each board's written ones are copied
    int topology = GOLHIP_TOPOLOGY_TORUS;
    int box_w = 0, box_h = 0;  // the soup box of init_random and search; 0, 0: the whole board
    std::string err;
};

namespace golhip {
namespace {

constexpr int64_t kSearchChunk = 65536;                     // soups per gol_batch_search launch, at most
constexpr int64_t kSearchChunkUpdates = (int64_t)1 << 44;  // cell updates per launch if no soup repeats, at most

int bfail(golhip_batch_t b, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (b)
        b->err = buf;
    else
        g_create_error = buf;
    return code;
}

#define BHIPCHK(b, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return bfail((b), e_ == hipErrorOutOfMemory ? GOLHIP_ERR_OOM : GOLHIP_ERR_HIP,         \
                         "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
    } while (0)

void batch_free(golhip_batch_t b) {
    if (hipSetDevice(b->device) != hipSuccess) return;
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->boards) (void)hipFree(b->boards);
    if (b->prev) (void)hipFree(b->prev);
    if (b->last_diff) (void)hipFree(b->last_diff);
    if (b->snap) (void)hipFree(b->snap);
    if (b->repeat_turn) (void)hipFree(b->repeat_turn);
    if (b->stage) (void)hipFree(b->stage);
    if (b->rules) (void)hipFree(b->rules);
    if (b->search_seeds) (void)hipFree(b->search_seeds);
    if (b->search_rules) (void)hipFree(b->search_rules);
    if (b->search_out) (void)hipFree(b->search_out);
    if (b->search_cycle) (void)hipFree(b->search_cycle);
    if (b->search_ash) (void)hipFree(b->search_ash);
    if (b->search_ash_turn) (void)hipFree(b->search_ash_turn);
    if (b->search_stage) (void)hipFree(b->search_stage);
    if (b->census_pat) (void)hipFree(b->census_pat);
    if (b->objects_host) (void)hipHostFree(b->objects_host);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    b->boards = b->prev = b->rules = b->snap = nullptr;
    b->last_diff = nullptr;
    b->repeat_turn = nullptr;
    b->stage = nullptr;
    b->search_seeds = nullptr;
    b->search_rules = nullptr;
    b->search_out = nullptr;
    b->search_cycle = nullptr;
    b->search_ash = nullptr;
    b->search_ash_turn = nullptr;
    b->search_stage = nullptr;
    b->search_stage_bytes = 0;
    b->census_pat = nullptr;
    b->objects_host = nullptr;
    b->objects_host_bytes = 0;
    b->stream = nullptr;
}

int batch_alloc(golhip_batch_t b) {
    BHIPCHK(b, hipSetDevice(b->device));
    hipDeviceProp_t prop;
    BHIPCHK(b, hipGetDeviceProperties(&prop, b->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bfail(b, GOLHIP_ERR_NODEV, "device %d is %s, libgolhip is built for gfx950", b->device,
                     prop.gcnArchName);
    BHIPCHK(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    const size_t bytes = sizeof(uint32_t) * (size_t)b->board_words * (size_t)b->nboards;
    BHIPCHK(b, hipMalloc(&b->boards, bytes));
    BHIPCHK(b, hipMemsetAsync(b->boards, 0, bytes, b->stream));
    // the stage: every board as bytes if that fits in kStageBytes (GOLHIP_STAGE_BYTES, read at
    // create, shrinks it: tests force chunked transfers and several launches per history call);
    // never less than one byte row or one uint32 per board (a generation of history, the counts)
    int64_t cap = kStageBytes;
    if (const char *e = std::getenv("GOLHIP_STAGE_BYTES")) cap = b->stage_limit = std::max<int64_t>(1, std::atoll(e));
    const int64_t floor_bytes = std::max<int64_t>(b->width, 4 * (int64_t)b->nboards);
    b->stage_bytes = std::max<int64_t>(floor_bytes, std::min<int64_t>(cap, b->width * b->height * b->nboards));
    BHIPCHK(b, hipMalloc(&b->stage, (size_t)b->stage_bytes));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

// A new set of boards: turn 0, no settle record, no repeat.
int boards_replaced(golhip_batch_t b) {
    b->turn = 0;
    if (b->last_diff)
        BHIPCHK(b, hipMemsetAsync(b->last_diff, 0, sizeof(unsigned long long) * (size_t)b->nboards, b->stream));
    if (b->repeat_turn)  // every byte 0xff: -1
        BHIPCHK(b, hipMemsetAsync(b->repeat_turn, 0xff, sizeof(int64_t) * (size_t)b->nboards, b->stream));
    return GOLHIP_OK;
}

// Boards [first, first + n) <-> host bytes, as one tall array of n * height byte rows cut into
// chunks the stage holds; a chunk is copied in one piece where the host rows are dense, else one
// 2-D copy per board it touches.
// The route itself, for n boards of the batch layout at `base` through a stage of stage_bytes: the
// batch's own boards through its stage (transfer), or the ash buffer of golhip_batch_search_census
// through that call's own stage (store only).  The strides have been checked.
int transfer_boards(golhip_batch_t b, uint32_t *base, int64_t n, uint8_t *host, size_t row_stride, size_t board_stride,
                    bool to_device, uint8_t *stage, int64_t stage_bytes) {
    const int64_t W = b->width, H = b->height;
    const bool dense = row_stride == (size_t)W && board_stride == (size_t)(W * H);
    const int64_t rows = n * H, cr = std::max<int64_t>(1, stage_bytes / W);
    for (int64_t r0 = 0; r0 < rows; r0 += cr) {
        const int64_t nr = std::min(cr, rows - r0);
        uint32_t *dev = base + r0 * b->wd;
        if (!to_device) BHIPCHK(b, launch_unpack(dev, b->wd, nr, W, stage, b->stream));
        for (int64_t r = r0; r < r0 + nr;) {  // the chunk's rows, board by board
            const int64_t bi = r / H, y = r - bi * H;
            const int64_t m = dense ? nr : std::min(H - y, r0 + nr - r);
            uint8_t *hp = host + (size_t)bi * board_stride + (size_t)y * row_stride;
            uint8_t *sp = stage + (r - r0) * W;
            if (to_device)
                BHIPCHK(b, hipMemcpy2DAsync(sp, (size_t)W, hp, row_stride, (size_t)W, (size_t)m, hipMemcpyHostToDevice,
                                            b->stream));
            else
                BHIPCHK(b, hipMemcpy2DAsync(hp, row_stride, sp, (size_t)W, (size_t)W, (size_t)m, hipMemcpyDeviceToHost,
                                            b->stream));
            r += m;
        }
        if (to_device) BHIPCHK(b, launch_pack(stage, nr, W, b->wd, dev, b->wd, b->stream));
        BHIPCHK(b, hipStreamSynchronize(b->stream));
    }
    return GOLHIP_OK;
}

int transfer(golhip_batch_t b, int first, int n, uint8_t *host, size_t row_stride, size_t board_stride,
             bool to_device) {
    if (!host) return bfail(b, GOLHIP_ERR_ARG, "buffer is null");
    if (first < 0 || n < 1 || (int64_t)first + n > b->nboards)
        return bfail(b, GOLHIP_ERR_ARG, "boards [%d, %lld) outside the batch's %d boards", first,
                     (long long)first + n, b->nboards);
    const int64_t W = b->width, H = b->height;
    if (row_stride < (size_t)W) return bfail(b, GOLHIP_ERR_ARG, "row_stride %zu < width %lld", row_stride, (long long)W);
    if (board_stride < (size_t)(H - 1) * row_stride + (size_t)W)
        return bfail(b, GOLHIP_ERR_ARG, "board_stride %zu < the %lld rows of a board", board_stride, (long long)H);
    BHIPCHK(b, hipSetDevice(b->device));
    return transfer_boards(b, b->boards + (int64_t)first * b->board_words, n, host, row_stride, board_stride, to_device,
                           b->stage, b->stage_bytes);
}

// What the next step launches: 0 gol_batch (uniform B3/S23), 1 gol_batch_rule constant-folded, 2 its
// table form, 3 the table form with per-board rules.  On a plane: 0 B3/S23's rule step, 2 the table
// form for every other uniform rule (the plane has no constant-folded kernels), 3 per-board rules.
int kernel_form(const golhip_batch *b) {
    if (b->per_board) return 3;
    if (b->rule.birth == kLifeBirth && b->rule.survive == kLifeSurvive) return 0;
    if (b->topology == GOLHIP_TOPOLOGY_PLANE) return 2;
    return rule_catalogued(b->rule.birth, b->rule.survive) ? 1 : 2;
}

// The soup box in cells: centred, the whole board when none is set.
SoupBox soup_box(const golhip_batch *b) {
    if (b->box_w == 0) return SoupBox{0, 0, (int32_t)b->width, (int32_t)b->height};
    return SoupBox{(int32_t)((b->width - b->box_w) / 2), (int32_t)((b->height - b->box_h) / 2), b->box_w, b->box_h};
}

// The settle record (last_diff, prev) and the period record (repeat_turn, snap) describe the boards
// under one rule.
int rule_change_allowed(golhip_batch_t b) {
    if (b->track && b->turn > 0)
        return bfail(b, GOLHIP_ERR_STATE, "settle tracking is on at turn %lld: the settle record holds under one rule, "
                     "change the rule at turn 0 (after a load)", (long long)b->turn);
    if (b->track_period && b->turn > 0)
        return bfail(b, GOLHIP_ERR_STATE, "period tracking is on at turn %lld: a repeat means a cycle under one rule "
                     "only, change the rule at turn 0 (after a load)", (long long)b->turn);
    return GOLHIP_OK;
}

}  // namespace

// The exact pass behind a chunk's search launch: gol_batch_cycle under B3/S23's rule step for a uniform
// B3/S23, in the table form for every other rule and for per-soup rules (a catalogue rule too: the
// pass has no constant-folded kernels).  A missing kernel is an error.
hipError_t launch_batch_cycle(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s) {
    const BatchSearchParams &sp = cp.bp.s;
    const SoupBox &bx = cp.bp.box;
    if (sp.max_turns < 1 || sp.max_turns > kSearchMaxTurns || nsoups < 1 || !sp.out || !cp.cycle_start ||
        (cp.ash && !cp.ash_turn) ||
        (sp.wd != 4 && sp.wd != 8 && sp.wd != 16) || sp.width < 64 || sp.width % 64 != 0 || sp.width > 32 * sp.wd ||
        (sp.width & (sp.width - 1)) != 0)
        return hipErrorInvalidValue;
    if (bx.w < 1 || bx.h < 1 || bx.x0 < 0 || bx.y0 < 0 || bx.x0 + bx.w > sp.width || bx.y0 + bx.h > 4 * W * R)
        return hipErrorInvalidValue;
    if (!sp.rules && ((sp.rule.birth | sp.rule.survive) & ~kRuleMaskBits)) return hipErrorInvalidValue;
    if (!sp.rules && sp.rule.birth == kLifeBirth && sp.rule.survive == kLifeSurvive)
        return launch_batch_cycle_life(W, R, nsoups, cp, s);
    return launch_batch_cycle_table(W, R, nsoups, cp, s);
}

}  // namespace golhip

using namespace golhip;

// ================================================================================ C ABI ====
extern "C" {

int golhip_batch_create(int width, int height, int nboards, int device, golhip_batch_t *out) {
    if (!out) return bfail(nullptr, GOLHIP_ERR_ARG, "out is null");
    *out = nullptr;
    int W = 0, R = 0;
    const int64_t L = width >= 1 && width <= 512 ? lcm64(width, 128) : 0;
    if (L != 128 && L != 256 && L != 512)
        return bfail(nullptr, GOLHIP_ERR_ARG,
                     "batch width %d: the torus lcm(width, 128) must be 128, 256 or 512 cells wide", width);
    if (!stencil_board_shape(height, (int32_t)(L / 32), &W, &R))
        return bfail(nullptr, GOLHIP_ERR_ARG, "batch height %d: one of 4, 8, 16, 32, 64, 128, 256, 512 rows", height);
    if (nboards < 1) return bfail(nullptr, GOLHIP_ERR_ARG, "batch nboards %d: at least 1", nboards);
    if (device < 0) return bfail(nullptr, GOLHIP_ERR_ARG, "batch device %d", device);
    golhip_batch *b = new golhip_batch;
    b->width = width;
    b->height = height;
    b->L = L;
    b->wd = (int32_t)(L / 32);
    b->W = W;
    b->R = R;
    b->nboards = nboards;
    b->device = device;
    b->board_words = (int64_t)height * b->wd;
    const int rc = batch_alloc(b);
    if (rc) {
        g_create_error = b->err;
        batch_free(b);  // nothing is leaked
        delete b;
        return rc;
    }
    *out = b;
    return GOLHIP_OK;
}

int golhip_batch_destroy(golhip_batch_t b) {
    if (!b) return GOLHIP_ERR_ARG;
    batch_free(b);
    delete b;
    return GOLHIP_OK;
}

const char *golhip_batch_last_error(golhip_batch_t b) { return b ? b->err.c_str() : g_create_error.c_str(); }

int golhip_batch_load_bytes(golhip_batch_t b, int first, int n, const uint8_t *cells, size_t row_stride,
                            size_t board_stride) {
    if (!b) return GOLHIP_ERR_ARG;
    const int rc = transfer(b, first, n, const_cast<uint8_t *>(cells), row_stride, board_stride, true);
    if (rc) return rc;
    return boards_replaced(b);
}

int golhip_batch_store_bytes(golhip_batch_t b, int first, int n, uint8_t *out, size_t row_stride,
                             size_t board_stride) {
    if (!b) return GOLHIP_ERR_ARG;
    return transfer(b, first, n, out, row_stride, board_stride, false);
}

int golhip_batch_init_random(golhip_batch_t b, const uint64_t *seeds, uint64_t seed0, uint32_t density_q32) {
    if (!b) return GOLHIP_ERR_ARG;
    if (b->width % 64 != 0)
        return bfail(b, GOLHIP_ERR_ARG, "init_random needs width %% 64 == 0 (width %lld)", (long long)b->width);
    BHIPCHK(b, hipSetDevice(b->device));
    if (!seeds) {
        BHIPCHK(b, launch_batch_init_random(b->boards, b->board_words, b->nboards, b->height, b->width, b->wd,
                                            nullptr, seed0, density_q32, b->stream));
        if (b->box_w)  // the boxed soup: the full-board soup with the cells outside the box cleared
            BHIPCHK(b, launch_batch_clip_box(b->boards, b->board_words, b->nboards, b->height, b->width, b->wd,
                                             soup_box(b), b->stream));
    } else {  // the seeds through the stage, a chunk of boards at a time
        uint64_t *dseeds = reinterpret_cast<uint64_t *>(b->stage);
        const int64_t cb = std::max<int64_t>(1, b->stage_bytes / (int64_t)sizeof(uint64_t));
        for (int64_t i = 0; i < b->nboards; i += cb) {
            const int64_t nb = std::min<int64_t>(cb, b->nboards - i);
            BHIPCHK(b, hipMemcpyAsync(dseeds, seeds + i, sizeof(uint64_t) * (size_t)nb, hipMemcpyHostToDevice,
                                      b->stream));
            BHIPCHK(b, launch_batch_init_random(b->boards + i * b->board_words, b->board_words, nb, b->height,
                                                b->width, b->wd, dseeds, 0, density_q32, b->stream));
            if (b->box_w)
                BHIPCHK(b, launch_batch_clip_box(b->boards + i * b->board_words, b->board_words, nb, b->height,
                                                 b->width, b->wd, soup_box(b), b->stream));
            BHIPCHK(b, hipStreamSynchronize(b->stream));
        }
    }
    const int rc = boards_replaced(b);
    if (rc) return rc;
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

int golhip_batch_step(golhip_batch_t b, int64_t turns, uint32_t *history, size_t board_stride) {
    if (!b) return GOLHIP_ERR_ARG;
    if (turns < 0) return bfail(b, GOLHIP_ERR_ARG, "turns %lld < 0", (long long)turns);
    if (turns == 0) return GOLHIP_OK;
    if (history && board_stride < (size_t)turns)
        return bfail(b, GOLHIP_ERR_ARG, "board_stride %zu < turns %lld", board_stride, (long long)turns);
    BHIPCHK(b, hipSetDevice(b->device));
    // a launch is at most kBoardMaxK deep, and with history no deeper than the stage holds counts
    // for: nboards * K * 4 bytes
    int64_t kmax = kBoardMaxK;
    if (history) kmax = std::max<int64_t>(1, std::min<int64_t>(kmax, b->stage_bytes / (4 * (int64_t)b->nboards)));
    BatchParams p{};
    p.boards = b->boards;
    p.board_pitch = b->board_words;
    p.wd = b->wd;
    p.width = (int32_t)b->width;
    p.hist = history ? reinterpret_cast<uint32_t *>(b->stage) : nullptr;
    p.prev = b->track ? b->prev : nullptr;
    p.last_diff = b->track ? b->last_diff : nullptr;
    const int form = kernel_form(b);
    const bool plane = b->topology == GOLHIP_TOPOLOGY_PLANE;
    for (int64_t done = 0; done < turns;) {
        const int K = (int)std::min<int64_t>(kmax, turns - done);
        p.t0 = b->turn;
        if (plane && b->track_period) {  // the plane kernels: every rule form, B3/S23 included
            const BatchPeriodParams pp{p, b->rule, b->per_board ? b->rules : nullptr, b->snap, b->repeat_turn};
            BHIPCHK(b, launch_plane_period(K, b->W, b->R, b->nboards, pp, b->stream));
        } else if (plane) {
            const BatchRuleParams rp{p, b->rule, b->per_board ? b->rules : nullptr};
            BHIPCHK(b, launch_plane_rule(K, b->W, b->R, b->nboards, rp, b->stream));
        } else if (b->track_period) {  // every rule form, B3/S23 included: the period kernels
            const BatchPeriodParams pp{p, b->rule, b->per_board ? b->rules : nullptr, b->snap, b->repeat_turn};
            BHIPCHK(b, launch_batch_period(K, b->W, b->R, b->nboards, pp, b->stream));
        } else if (form == 0) {
            BHIPCHK(b, launch_batch_board(K, b->W, b->R, b->nboards, p, b->stream));
        } else {  // a missing kernel is an error, never gol_batch
            const BatchRuleParams rp{p, b->rule, b->per_board ? b->rules : nullptr};
            BHIPCHK(b, launch_batch_rule(K, b->W, b->R, b->nboards, rp, b->stream));
        }
        if (history) {
            BHIPCHK(b, hipMemcpy2DAsync(history + done, board_stride * sizeof(uint32_t), p.hist, (size_t)K * 4,
                                        (size_t)K * 4, (size_t)b->nboards, hipMemcpyDeviceToHost, b->stream));
            BHIPCHK(b, hipStreamSynchronize(b->stream));  // the next launch rewrites the stage
        }
        b->turn += K;
        done += K;
    }
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

int golhip_batch_alive_counts(golhip_batch_t b, uint32_t *out) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!out) return bfail(b, GOLHIP_ERR_ARG, "out is null");
    BHIPCHK(b, hipSetDevice(b->device));
    uint32_t *d = reinterpret_cast<uint32_t *>(b->stage);  // stage_bytes >= 4 * nboards
    BHIPCHK(b, launch_batch_popcount(b->boards, b->board_words, b->nboards, b->height, b->width, b->wd, d, b->stream));
    BHIPCHK(b, hipMemcpyAsync(out, d, sizeof(uint32_t) * (size_t)b->nboards, hipMemcpyDeviceToHost, b->stream));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

int golhip_batch_track_settle(golhip_batch_t b, int enable) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!enable) {
        b->track = false;
        return GOLHIP_OK;
    }
    if (b->track) return GOLHIP_OK;
    if (b->track_period)
        return bfail(b, GOLHIP_ERR_STATE, "period tracking is on: settle tracking and period tracking exclude each "
                     "other (golhip_batch_track_period(b, 0) first)");
    if (b->turn != 0)
        return bfail(b, GOLHIP_ERR_STATE, "settle tracking starts at turn 0 (turn %lld): enable it after a load, "
                     "before the first step", (long long)b->turn);
    BHIPCHK(b, hipSetDevice(b->device));
    if (!b->prev) BHIPCHK(b, hipMalloc(&b->prev, sizeof(uint32_t) * (size_t)b->board_words * (size_t)b->nboards));
    if (!b->last_diff) BHIPCHK(b, hipMalloc(&b->last_diff, sizeof(unsigned long long) * (size_t)b->nboards));
    BHIPCHK(b, hipMemsetAsync(b->last_diff, 0, sizeof(unsigned long long) * (size_t)b->nboards, b->stream));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    b->track = true;
    return GOLHIP_OK;
}

int golhip_batch_settled(golhip_batch_t b, int64_t *out) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!out) return bfail(b, GOLHIP_ERR_ARG, "out is null");
    if (!b->track) return bfail(b, GOLHIP_ERR_STATE, "settle tracking is off (golhip_batch_track_settle)");
    BHIPCHK(b, hipSetDevice(b->device));
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "last_diff is copied into out");
    BHIPCHK(b, hipMemcpyAsync(out, b->last_diff, sizeof(int64_t) * (size_t)b->nboards, hipMemcpyDeviceToHost,
                              b->stream));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    // board(t) != board(t - 2) exactly for t in [2, D]: the settle turn is D + 1 (2 when nothing
    // ever differed), known once that turn has been run
    for (int i = 0; i < b->nboards; ++i) {
        const int64_t t = std::max<int64_t>(out[i], 1) + 1;
        out[i] = t <= b->turn ? t : -1;
    }
    return GOLHIP_OK;
}

int golhip_batch_track_period(golhip_batch_t b, int enable) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!enable) {
        b->track_period = false;
        return GOLHIP_OK;
    }
    if (b->track_period) return GOLHIP_OK;
    if (b->track)
        return bfail(b, GOLHIP_ERR_STATE, "settle tracking is on: period tracking and settle tracking exclude each "
                     "other (golhip_batch_track_settle(b, 0) first)");
    if (b->turn != 0)
        return bfail(b, GOLHIP_ERR_STATE, "period tracking starts at turn 0 (turn %lld): board(0) is the first "
                     "snapshot, enable it after a load, before the first step", (long long)b->turn);
    BHIPCHK(b, hipSetDevice(b->device));
    if (!b->snap) BHIPCHK(b, hipMalloc(&b->snap, sizeof(uint32_t) * (size_t)b->board_words * (size_t)b->nboards));
    if (!b->repeat_turn) BHIPCHK(b, hipMalloc(&b->repeat_turn, sizeof(int64_t) * (size_t)b->nboards));
    BHIPCHK(b, hipMemsetAsync(b->repeat_turn, 0xff, sizeof(int64_t) * (size_t)b->nboards, b->stream));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    b->track_period = true;
    return GOLHIP_OK;
}

int golhip_batch_periods(golhip_batch_t b, int64_t *repeat_turn, int64_t *period) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!b->track_period) return bfail(b, GOLHIP_ERR_STATE, "period tracking is off (golhip_batch_track_period)");
    if (!repeat_turn && !period) return GOLHIP_OK;
    BHIPCHK(b, hipSetDevice(b->device));
    std::vector<int64_t> own;
    int64_t *rt = repeat_turn;
    if (!rt) {
        own.resize((size_t)b->nboards);
        rt = own.data();
    }
    BHIPCHK(b, hipMemcpyAsync(rt, b->repeat_turn, sizeof(int64_t) * (size_t)b->nboards, hipMemcpyDeviceToHost,
                              b->stream));
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    if (period) {  // t - s(t), s(t) = 2^floor(log2 t) - 1: the snapshot turn of the window t lies in
        for (int i = 0; i < b->nboards; ++i) {
            const int64_t t = rt[i];
            int64_t top = 1;
            while (t > 0 && 2 * top <= t) top *= 2;
            period[i] = t > 0 ? t - (top - 1) : -1;
        }
    }
    return GOLHIP_OK;
}

int golhip_batch_turn(golhip_batch_t b, int64_t *out) {
    if (!b || !out) return GOLHIP_ERR_ARG;
    *out = b->turn;
    return GOLHIP_OK;
}

int golhip_batch_set_rule_masks(golhip_batch_t b, uint32_t birth, uint32_t survive) {
    if (!b) return GOLHIP_ERR_ARG;
    if ((birth | survive) & ~kRuleMaskBits)
        return bfail(b, GOLHIP_ERR_ARG, "rule masks birth=0x%x survive=0x%x: bits above 8 (a cell has 8 neighbours)",
                     birth, survive);
    if (!b->per_board && birth == b->rule.birth && survive == b->rule.survive) return GOLHIP_OK;
    const int rc = rule_change_allowed(b);
    if (rc) return rc;
    b->rule.birth = birth;
    b->rule.survive = survive;
    b->per_board = false;
    return GOLHIP_OK;
}

int golhip_batch_set_rule(golhip_batch_t b, const char *rule) {
    if (!b) return GOLHIP_ERR_ARG;
    uint32_t birth = 0, survive = 0;
    if (golhip_parse_rule(rule, &birth, &survive) != GOLHIP_OK) return bfail(b, GOLHIP_ERR_ARG, "%s", g_create_error.c_str());
    return golhip_batch_set_rule_masks(b, birth, survive);
}

int golhip_batch_get_rule(golhip_batch_t b, uint32_t *birth, uint32_t *survive) {
    if (!b || !birth || !survive) return GOLHIP_ERR_ARG;
    if (b->per_board)
        return bfail(b, GOLHIP_ERR_STATE, "the boards have rules of their own (golhip_batch_get_rules)");
    *birth = b->rule.birth;
    *survive = b->rule.survive;
    return GOLHIP_OK;
}

int golhip_batch_set_rules(golhip_batch_t b, const uint32_t *birth, const uint32_t *survive) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!birth != !survive) return bfail(b, GOLHIP_ERR_ARG, "birth and survive: both arrays, or both null");
    if (birth) {
        for (int i = 0; i < b->nboards; ++i) {
            if ((birth[i] | survive[i]) & ~kRuleMaskBits)
                return bfail(b, GOLHIP_ERR_ARG, "board %d: rule masks birth=0x%x survive=0x%x: bits above 8 (a cell "
                             "has 8 neighbours)", i, birth[i], survive[i]);
        }
    }
    if (!birth && !b->per_board) return GOLHIP_OK;
    int rc = rule_change_allowed(b);
    if (rc) return rc;
    if (!birth) {  // back to the uniform rule
        b->per_board = false;
        return GOLHIP_OK;
    }
    BHIPCHK(b, hipSetDevice(b->device));
    const size_t n = (size_t)b->nboards;
    if (!b->rules) BHIPCHK(b, hipMalloc(&b->rules, 2 * sizeof(uint32_t) * n));
    std::vector<uint32_t> pairs(2 * n);
    for (size_t i = 0; i < n; ++i) pairs[2 * i] = birth[i], pairs[2 * i + 1] = survive[i];
    // through the stage, as many pairs at a time as it holds (>= 4 nboards bytes: at most two chunks)
    const size_t cp = std::max<size_t>(1, (size_t)b->stage_bytes / (2 * sizeof(uint32_t)));
    b->per_board = false;  // a failed upload leaves the uniform rule
    for (size_t i = 0; i < n; i += cp) {
        const size_t bytes = 2 * sizeof(uint32_t) * std::min(cp, n - i);
        BHIPCHK(b, hipMemcpyAsync(b->stage, pairs.data() + 2 * i, bytes, hipMemcpyHostToDevice, b->stream));
        BHIPCHK(b, hipMemcpyAsync(b->rules + 2 * i, b->stage, bytes, hipMemcpyDeviceToDevice, b->stream));
        BHIPCHK(b, hipStreamSynchronize(b->stream));
    }
    b->rules_host.swap(pairs);
    b->per_board = true;
    return GOLHIP_OK;
}

int golhip_batch_get_rules(golhip_batch_t b, uint32_t *birth, uint32_t *survive) {
    if (!b) return GOLHIP_ERR_ARG;
    if (!birth || !survive) return bfail(b, GOLHIP_ERR_ARG, "out is null");
    for (int i = 0; i < b->nboards; ++i) {
        birth[i] = b->per_board ? b->rules_host[2 * (size_t)i] : b->rule.birth;
        survive[i] = b->per_board ? b->rules_host[2 * (size_t)i + 1] : b->rule.survive;
    }
    return GOLHIP_OK;
}

// golhip_batch_search (exact == false: cycle_start is not looked at) and golhip_batch_search_exact: the
// same checks, chunks and search launches; the exact call adds gol_batch_cycle behind each chunk's
// search launch and one more copy.  golhip_batch_search_census (sc set) is the exact call whose pass also
// hands a board on each soup's cycle to the census, chunk by chunk in stream order: the search
// launch, the chunk's ash zeroed, gol_batch_cycle with the ash buffer, the census over that buffer,
// the ash unpacked if it is asked for.
struct SearchCensus {
    const golhip_pattern_t *patterns;
    int npat;
    int64_t *ash_turn;
    uint32_t *counts, *residue;
    uint8_t *ash_cells;
};
// golhip_batch_search_objects (so set) is the same call with gol_batch_objects over the ash buffer in the
// census's place.
struct SearchObjects {
    int max_objects, reach;
    int64_t *ash_turn;
    int32_t *nobjects;
    golhip_object_t *objects;
};
constexpr int64_t kAshBytes = (int64_t)64 << 20;  // the ash buffer of a chunk, at most
constexpr int64_t kObjectsStageFloor = 4 + (int64_t)sizeof(golhip_object_t);  // a count and one record
static int objects_check(golhip_batch_t b, int max_objects, int reach);
static int objects_boards(golhip_batch_t b, const uint32_t *base, int64_t nboards, int max_objects, int reach,
                          int32_t *nobjects, golhip_object_t *objects);

// The stage of golhip_batch_search_census and of the objects calls: `need` bytes, at most 64 MiB; the test
// hook shrinks it as it shrinks the batch's, never below floor_bytes; it only grows.
static int reserve_search_stage(golhip_batch_t b, int64_t need, int64_t floor_bytes) {
    need = std::min(need, kAshBytes);
    if (b->stage_limit) need = std::min(need, std::max<int64_t>(b->stage_limit, floor_bytes));
    if (need > b->search_stage_bytes) {
        if (b->search_stage) BHIPCHK(b, hipFree(b->search_stage));
        b->search_stage = nullptr;
        b->search_stage_bytes = 0;
        BHIPCHK(b, hipMalloc(&b->search_stage, (size_t)need));
        b->search_stage_bytes = need;
    }
    return GOLHIP_OK;
}
static int census_check(golhip_batch_t b, const golhip_pattern_t *patterns, int npat);
static int census_boards(golhip_batch_t b, const uint32_t *base, int64_t nboards, int npat, uint32_t *counts,
                         uint32_t *residue, uint32_t *stage, int64_t cap);

static int search_run(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds, uint64_t seed0, uint32_t density_q32,
                      int64_t max_turns, const uint32_t *birth, const uint32_t *survive, golhip_soup_t *out,
                      int64_t *cycle_start, bool exact, const SearchCensus *sc = nullptr,
                      const SearchObjects *so = nullptr) {
    if (!b) return GOLHIP_ERR_ARG;
    const bool ashed = sc || so;
    int64_t *const ash_turn = sc ? sc->ash_turn : so ? so->ash_turn : nullptr;
    if (b->width % 64 != 0)
        return bfail(b, GOLHIP_ERR_ARG, "search needs width %% 64 == 0, as init_random (width %lld)", (long long)b->width);
    if (max_turns < 1 || max_turns > kSearchMaxTurns)
        return bfail(b, GOLHIP_ERR_ARG, "search max_turns %lld: 1 to %lld", (long long)max_turns,
                     (long long)kSearchMaxTurns);
    if (nsoups < 0) return bfail(b, GOLHIP_ERR_ARG, "search nsoups %lld < 0", (long long)nsoups);
    if (!birth != !survive) return bfail(b, GOLHIP_ERR_ARG, "birth and survive: both arrays, or both null");
    if (birth) {
        for (int64_t i = 0; i < nsoups; ++i) {
            if ((birth[i] | survive[i]) & ~kRuleMaskBits)
                return bfail(b, GOLHIP_ERR_ARG, "soup %lld: rule masks birth=0x%x survive=0x%x: bits above 8 (a cell "
                             "has 8 neighbours)", (long long)i, birth[i], survive[i]);
        }
    }
    if (sc) {  // the census's checks, in golhip_batch_census's words
        if (sc->npat < 0 || sc->npat > kCensusMaxPatterns)
            return bfail(b, GOLHIP_ERR_ARG, "census npat %d: 0 to %d patterns", sc->npat, kCensusMaxPatterns);
        if (sc->npat > 0 && !sc->patterns)
            return bfail(b, GOLHIP_ERR_ARG, "census patterns is null with npat %d", sc->npat);
        if (!sc->counts && !sc->residue && !sc->ash_cells)
            return bfail(b, GOLHIP_ERR_ARG, "census counts, residue and ash_cells are all null");
        if (sc->counts && sc->npat == 0)
            return bfail(b, GOLHIP_ERR_ARG, "census npat 0 with counts: counts has no columns, pass null");
        const int rc = census_check(b, sc->patterns, sc->npat);
        if (rc) return rc;
    }
    if (so) {  // the checks of golhip_batch_objects, in its words
        const int rc = objects_check(b, so->max_objects, so->reach);
        if (rc) return rc;
    }
    if (nsoups == 0) return GOLHIP_OK;
    if (!out) return bfail(b, GOLHIP_ERR_ARG, "out is null");
    if (exact && !cycle_start) return bfail(b, GOLHIP_ERR_ARG, "cycle_start is null");
    if (ashed && !ash_turn) return bfail(b, GOLHIP_ERR_ARG, "ash_turn is null");
    if (so && !so->nobjects) return bfail(b, GOLHIP_ERR_ARG, "objects nobjects is null");
    static_assert(sizeof(golhip_soup_t) == 32 && sizeof(SoupRecord) == 32, "a soup's record is 32 bytes");
    static_assert(offsetof(golhip_soup_t, repeat_turn) == offsetof(SoupRecord, repeat_turn) &&
                      offsetof(golhip_soup_t, period) == offsetof(SoupRecord, period) &&
                      offsetof(golhip_soup_t, stop_turn) == offsetof(SoupRecord, stop_turn) &&
                      offsetof(golhip_soup_t, population) == offsetof(SoupRecord, population) &&
                      offsetof(golhip_soup_t, reserved) == offsetof(SoupRecord, reserved),
                  "the kernel's record is golhip_soup_t");
    BHIPCHK(b, hipSetDevice(b->device));
    if (!b->search_seeds) BHIPCHK(b, hipMalloc(&b->search_seeds, sizeof(uint64_t) * (size_t)kSearchChunk));
    if (!b->search_rules) BHIPCHK(b, hipMalloc(&b->search_rules, 2 * sizeof(uint32_t) * (size_t)kSearchChunk));
    if (!b->search_out) BHIPCHK(b, hipMalloc(&b->search_out, sizeof(SoupRecord) * (size_t)kSearchChunk));
    if (!b->search_cycle) BHIPCHK(b, hipMalloc(&b->search_cycle, sizeof(int64_t) * (size_t)kSearchChunk));
    // a chunk: at most kSearchChunk soups and at most 2^44 cell updates if no soup repeats, at least 1
    int64_t chunk = std::max<int64_t>(
        1, std::min<int64_t>(kSearchChunk, kSearchChunkUpdates / (b->width * b->height * max_turns)));
    if (ashed) {  // and no more soups than the ash buffer holds boards: 64 MiB, at least one board
        const int64_t board_bytes = (int64_t)sizeof(uint32_t) * b->board_words;
        const int64_t ash_boards = std::max<int64_t>(1, std::min<int64_t>(kSearchChunk, kAshBytes / board_bytes));
        if (!b->search_ash) BHIPCHK(b, hipMalloc(&b->search_ash, (size_t)(ash_boards * board_bytes)));
        if (!b->search_ash_turn) BHIPCHK(b, hipMalloc(&b->search_ash_turn, sizeof(int64_t) * (size_t)kSearchChunk));
        chunk = std::min(chunk, ash_boards);
        // The chunk's results come back through a stage of the call's own, not the batch's, which is sized
        // by nboards and a search runs on a batch of one board: a chunk's counts and residues, and
        // its cells if they are asked for, at most 64 MiB; it only grows.
        const int64_t most = std::min(chunk, nsoups);
        if (sc) {
            int64_t need = 4 * most * ((sc->counts ? sc->npat : 0) + 1);
            if (sc->ash_cells) need = std::max(need, most * b->width * b->height);
            // the test hook shrinks this stage as it shrinks the batch's: never below a byte row or a uint32
            const int rc = reserve_search_stage(b, need, std::max<int64_t>(b->width, 4));
            if (rc) return rc;
        }
        if (sc && sc->npat > 0 && (sc->counts || sc->residue)) {
            if (!b->census_pat)
                BHIPCHK(b, hipMalloc(&b->census_pat, sizeof(CensusPattern) * (size_t)kCensusMaxPatterns));
            BHIPCHK(b, hipMemcpyAsync(b->census_pat, sc->patterns, sizeof(CensusPattern) * (size_t)sc->npat,
                                      hipMemcpyHostToDevice, b->stream));
        }
    }
    BatchSearchParams sp{};
    sp.density = density_q32;
    sp.wd = b->wd;
    sp.width = (int32_t)b->width;
    sp.max_turns = (int32_t)max_turns;
    sp.rule = b->rule;  // the uniform rule; the handle's per-board rules belong to its boards
    sp.rules = birth ? b->search_rules : nullptr;
    sp.out = b->search_out;
    // the plane, or a box on either topology: gol_plane_search; a torus of whole-board soups runs
    // gol_batch_search as before
    const bool boxed = b->topology == GOLHIP_TOPOLOGY_PLANE || b->box_w != 0;
    std::vector<uint32_t> pairs;
    for (int64_t i = 0; i < nsoups; i += chunk) {
        const int64_t n = std::min(chunk, nsoups - i);
        if (seeds) {
            BHIPCHK(b, hipMemcpyAsync(b->search_seeds, seeds + i, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice,
                                      b->stream));
            sp.seeds = b->search_seeds;
        } else {
            sp.seed0 = seed0 + (uint64_t)i;
        }
        if (birth) {
            pairs.resize(2 * (size_t)n);
            for (int64_t j = 0; j < n; ++j) pairs[2 * j] = birth[i + j], pairs[2 * j + 1] = survive[i + j];
            BHIPCHK(b, hipMemcpyAsync(b->search_rules, pairs.data(), 2 * sizeof(uint32_t) * (size_t)n,
                                      hipMemcpyHostToDevice, b->stream));
        }
        // a missing kernel is an error
        if (boxed) {
            const BatchBoxSearchParams bp{sp, soup_box(b), b->topology == GOLHIP_TOPOLOGY_PLANE ? 1 : 0};
            BHIPCHK(b, launch_plane_search(b->W, b->R, (int)n, bp, b->stream));
        } else {
            BHIPCHK(b, launch_batch_search(b->W, b->R, (int)n, sp, b->stream));
        }
        BHIPCHK(b, hipMemcpyAsync(out + i, b->search_out, sizeof(SoupRecord) * (size_t)n, hipMemcpyDeviceToHost,
                                  b->stream));
        if (exact) {  // the second pass reads the chunk's records on the device (stream order)
            BatchCycleParams cp{{sp, soup_box(b), b->topology == GOLHIP_TOPOLOGY_PLANE ? 1 : 0}, b->search_cycle};
            if (ashed) {  // a soup without a repeat writes no row: its ash is the empty board
                BHIPCHK(b, hipMemsetAsync(b->search_ash, 0, sizeof(uint32_t) * (size_t)(n * b->board_words), b->stream));
                cp.ash = b->search_ash;
                cp.ash_turn = b->search_ash_turn;
            }
            BHIPCHK(b, launch_batch_cycle(b->W, b->R, (int)n, cp, b->stream));
            BHIPCHK(b, hipMemcpyAsync(cycle_start + i, b->search_cycle, sizeof(int64_t) * (size_t)n,
                                      hipMemcpyDeviceToHost, b->stream));
        }
        if (so) {  // the empty ash of a soup without a repeat has no cluster: nobjects 0
            BHIPCHK(b, hipMemcpyAsync(ash_turn + i, b->search_ash_turn, sizeof(int64_t) * (size_t)n,
                                      hipMemcpyDeviceToHost, b->stream));
            const int rc = objects_boards(b, b->search_ash, n, so->max_objects, so->reach, so->nobjects + i,
                                          so->objects ? so->objects + i * so->max_objects : nullptr);
            if (rc) return rc;
        }
        if (sc) {
            BHIPCHK(b, hipMemcpyAsync(ash_turn + i, b->search_ash_turn, sizeof(int64_t) * (size_t)n,
                                      hipMemcpyDeviceToHost, b->stream));
            uint32_t *res = sc->residue ? sc->residue + i : nullptr;
            if (sc->npat > 0 && (sc->counts || res)) {
                const int rc = census_boards(b, b->search_ash, n, sc->npat,
                                             sc->counts ? sc->counts + i * sc->npat : nullptr, res,
                                             reinterpret_cast<uint32_t *>(b->search_stage), b->search_stage_bytes / 4);
                if (rc) return rc;
            } else if (res) {  // no pattern: nothing is covered, the residue is the ash's live cells
                uint32_t *d = reinterpret_cast<uint32_t *>(b->search_stage);
                const int64_t cb = std::max<int64_t>(1, b->search_stage_bytes / 4);
                for (int64_t j = 0; j < n; j += cb) {
                    const int64_t nb = std::min<int64_t>(cb, n - j);
                    BHIPCHK(b, launch_batch_popcount(b->search_ash + j * b->board_words, b->board_words, nb, b->height,
                                                     b->width, b->wd, d, b->stream));
                    BHIPCHK(b, hipMemcpyAsync(res + j, d, sizeof(uint32_t) * (size_t)nb, hipMemcpyDeviceToHost, b->stream));
                    BHIPCHK(b, hipStreamSynchronize(b->stream));  // the next launch rewrites the stage
                }
            }
            if (sc->ash_cells) {
                const size_t cells = (size_t)(b->width * b->height);
                uint8_t *bytes = sc->ash_cells + (size_t)i * cells;
                const int rc = transfer_boards(b, b->search_ash, n, bytes, (size_t)b->width, cells, false,
                                               b->search_stage, b->search_stage_bytes);
                if (rc) return rc;
                for (size_t k = 0; k < (size_t)n * cells; ++k) bytes[k] &= 1;  // the unpack kernel's 255 -> 1
            }
            BHIPCHK(b, hipStreamSynchronize(b->stream));
            // a soup without a repeat: its cells are alive and none is explained
            if (res)
                for (int64_t j = 0; j < n; ++j)
                    if (out[i + j].repeat_turn < 0) res[j] = out[i + j].population;
        }
        BHIPCHK(b, hipStreamSynchronize(b->stream));  // the next chunk rewrites the buffers (and `pairs`)
    }
    return GOLHIP_OK;
}

int golhip_batch_search(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds, uint64_t seed0, uint32_t density_q32,
                        int64_t max_turns, const uint32_t *birth, const uint32_t *survive, golhip_soup_t *out) {
    return search_run(b, nsoups, seeds, seed0, density_q32, max_turns, birth, survive, out, nullptr, false);
}

int golhip_batch_search_exact(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds, uint64_t seed0,
                              uint32_t density_q32, int64_t max_turns, const uint32_t *birth, const uint32_t *survive,
                              golhip_soup_t *out, int64_t *cycle_start) {
    return search_run(b, nsoups, seeds, seed0, density_q32, max_turns, birth, survive, out, cycle_start, true);
}

int golhip_batch_search_census(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds, uint64_t seed0,
                               uint32_t density_q32, int64_t max_turns, const uint32_t *birth, const uint32_t *survive,
                               const golhip_pattern_t *patterns, int npat, golhip_soup_t *out, int64_t *cycle_start,
                               int64_t *ash_turn, uint32_t *counts, uint32_t *residue, uint8_t *ash_cells) {
    const SearchCensus sc{patterns, npat, ash_turn, counts, residue, ash_cells};
    return search_run(b, nsoups, seeds, seed0, density_q32, max_turns, birth, survive, out, cycle_start, true, &sc);
}

// The checks of golhip_batch_census's pattern list; the text names the pattern index and the offence.
static int census_check(golhip_batch_t b, const golhip_pattern_t *patterns, int npat) {
    for (int p = 0; p < npat; ++p) {
        const golhip_pattern_t &q = patterns[p];
        if (q.w < 1 || q.w > 32 || q.h < 1 || q.h > 32)
            return bfail(b, GOLHIP_ERR_ARG, "pattern %d: w %d, h %d: 1..32 each", p, q.w, q.h);
        if (q.w > b->width || q.h > b->height)
            return bfail(b, GOLHIP_ERR_ARG, "pattern %d: %d x %d is larger than the %lld x %lld board", p, q.w, q.h,
                         (long long)b->width, (long long)b->height);
        const uint32_t cols = q.w == 32 ? ~0u : (1u << q.w) - 1u;
        uint32_t live = 0;
        for (int r = 0; r < 32; ++r) {
            const uint32_t bits = q.alive[r] | q.care[r];
            if (r >= q.h && bits)
                return bfail(b, GOLHIP_ERR_ARG, "pattern %d: a bit in row %d, the pattern has %d rows", p, r, q.h);
            if (bits & ~cols)
                return bfail(b, GOLHIP_ERR_ARG, "pattern %d: row %d has a bit at a column >= w (%d)", p, r, q.w);
            if (q.alive[r] & ~q.care[r])
                return bfail(b, GOLHIP_ERR_ARG, "pattern %d: row %d: alive 0x%x is not a subset of care 0x%x", p, r,
                             q.alive[r], q.care[r]);
            live |= q.alive[r];
        }
        if (!live) return bfail(b, GOLHIP_ERR_ARG, "pattern %d: no live cell", p);
    }
    return GOLHIP_OK;
}

// The census of `nboards` boards of the batch layout at `base` -- the batch's own, or one chunk of
// golhip_batch_search_census's ash -- under the patterns already in b->census_pat (npat >= 1).  counts
// (nboards x npat) and residue (nboards) are host memory, either may be null.  The results come back
// through `stage`, device memory of cap >= 1 words: the batch's transfer stage, or the search's own.
static int census_boards(golhip_batch_t b, const uint32_t *base, int64_t nboards, int npat, uint32_t *counts,
                         uint32_t *residue, uint32_t *stage, int64_t cap) {
    BatchCensusParams cp{};
    cp.board_pitch = b->board_words;
    cp.wd = b->wd;
    cp.width = (int32_t)b->width;
    cp.height = (int32_t)b->height;
    cp.plane = b->topology == GOLHIP_TOPOLOGY_PLANE ? 1 : 0;
    // The results come back through the stage.  Where it holds a board's npat counts and its residue,
    // one pass: chunks of boards, each launch writing both.  A smaller stage (GOLHIP_STAGE_BYTES) takes the
    // counts in groups of patterns -- counts[.., p] does not depend on the other patterns -- and the
    // residue in a pass of its own over the whole list.
    const int64_t per_board = (counts ? npat : 0) + (residue ? 1 : 0);
    const bool one_pass = per_board <= cap;
    const int64_t pgroup = one_pass ? npat : std::min<int64_t>(npat, cap);
    for (int64_t p0 = 0; counts && p0 < npat; p0 += pgroup) {
        const int64_t np = std::min<int64_t>(pgroup, npat - p0);
        const bool both = one_pass && residue;
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(kSearchChunk, cap / (np + (both ? 1 : 0))));
        for (int64_t i = 0; i < nboards; i += chunk) {
            const int64_t n = std::min<int64_t>(chunk, nboards - i);
            cp.boards = base + i * b->board_words;
            cp.patterns = b->census_pat + p0;
            cp.npat = (int32_t)np;
            cp.counts = stage;
            cp.residue = both ? stage + n * np : nullptr;
            BHIPCHK(b, launch_batch_census((int)n, cp, b->stream));  // a missing kernel is an error
            BHIPCHK(b, hipMemcpy2DAsync(counts + i * npat + p0, sizeof(uint32_t) * (size_t)npat, stage,
                                        sizeof(uint32_t) * (size_t)np, sizeof(uint32_t) * (size_t)np, (size_t)n,
                                        hipMemcpyDeviceToHost, b->stream));
            if (both)
                BHIPCHK(b, hipMemcpyAsync(residue + i, cp.residue, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost,
                                          b->stream));
            BHIPCHK(b, hipStreamSynchronize(b->stream));  // the next launch rewrites the stage
        }
    }
    if (residue && !(counts && one_pass)) {
        const int64_t chunk = std::min<int64_t>(kSearchChunk, cap);
        for (int64_t i = 0; i < nboards; i += chunk) {
            const int64_t n = std::min<int64_t>(chunk, nboards - i);
            cp.boards = base + i * b->board_words;
            cp.patterns = b->census_pat;
            cp.npat = npat;
            cp.counts = nullptr;
            cp.residue = stage;
            BHIPCHK(b, launch_batch_census((int)n, cp, b->stream));
            BHIPCHK(b, hipMemcpyAsync(residue + i, stage, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, b->stream));
            BHIPCHK(b, hipStreamSynchronize(b->stream));
        }
    }
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

int golhip_batch_census(golhip_batch_t b, const golhip_pattern_t *patterns, int npat, uint32_t *counts,
                        uint32_t *residue) {
    if (!b) return GOLHIP_ERR_ARG;
    static_assert(sizeof(golhip_pattern_t) == 264 && sizeof(CensusPattern) == 264 &&
                      offsetof(golhip_pattern_t, alive) == offsetof(CensusPattern, alive) &&
                      offsetof(golhip_pattern_t, care) == offsetof(CensusPattern, care),
                  "the kernel's pattern is golhip_pattern_t");
    if (npat < 0 || npat > kCensusMaxPatterns)
        return bfail(b, GOLHIP_ERR_ARG, "census npat %d: 0 to %d patterns", npat, kCensusMaxPatterns);
    if (npat > 0 && !patterns) return bfail(b, GOLHIP_ERR_ARG, "census patterns is null with npat %d", npat);
    if (!counts && !residue) return bfail(b, GOLHIP_ERR_ARG, "census counts and residue are both null");
    int rc = census_check(b, patterns, npat);
    if (rc) return rc;
    if (npat == 0)  // nothing matches, nothing is covered; counts has no columns
        return residue ? golhip_batch_alive_counts(b, residue) : GOLHIP_OK;
    BHIPCHK(b, hipSetDevice(b->device));
    if (!b->census_pat) BHIPCHK(b, hipMalloc(&b->census_pat, sizeof(CensusPattern) * (size_t)kCensusMaxPatterns));
    BHIPCHK(b, hipMemcpyAsync(b->census_pat, patterns, sizeof(CensusPattern) * (size_t)npat, hipMemcpyHostToDevice,
                              b->stream));
    // the batch's stage: >= nboards >= 1 words
    return census_boards(b, b->boards, b->nboards, npat, counts, residue, reinterpret_cast<uint32_t *>(b->stage),
                         b->stage_bytes / 4);
}

// The checks of the objects calls; the text names the argument and its range.
static int objects_check(golhip_batch_t b, int max_objects, int reach) {
    if (max_objects < 1 || max_objects > kObjectsMax)
        return bfail(b, GOLHIP_ERR_ARG, "objects max_objects %d: 1 to %d", max_objects, kObjectsMax);
    if (reach != 1 && reach != 2) return bfail(b, GOLHIP_ERR_ARG, "objects reach %d: 1 or 2", reach);
    return GOLHIP_OK;
}

// The clusters of `nboards` boards of the batch layout at `base` -- the batch's own, or one chunk of
// golhip_batch_search_objects's ash.  nobjects (nboards) and objects (nboards x max_objects, or null) are
// host memory.  The results come back through the search stage, at most 64 MiB and what
// GOLHIP_STAGE_BYTES allows: where it holds a board's count and its max_objects records, chunks of
// boards, one launch each; a smaller stage takes one board at a time and its records in windows, one
// launch per window, as far as the board has clusters.  A launch writes only the records that exist,
// so a chunk's records go to pinned host memory first and each board's written ones from there.
static int objects_boards(golhip_batch_t b, const uint32_t *base, int64_t nboards, int max_objects, int reach,
                          int32_t *nobjects, golhip_object_t *objects) {
    static_assert(sizeof(golhip_object_t) == 32 && sizeof(ObjectRecord) == 32 &&
                      offsetof(golhip_object_t, population) == offsetof(ObjectRecord, population) &&
                      offsetof(golhip_object_t, flags) == offsetof(ObjectRecord, flags) &&
                      offsetof(golhip_object_t, hash) == offsetof(ObjectRecord, hash),
                  "the kernel's record is golhip_object_t");
    constexpr int64_t kRec = (int64_t)sizeof(golhip_object_t);
    const int64_t per_board = 4 + (objects ? kRec * max_objects : 0);
    int rc = reserve_search_stage(b, per_board * std::min<int64_t>(nboards, kSearchChunk), kObjectsStageFloor);
    if (rc) return rc;
    const int64_t cap = b->search_stage_bytes;
    const int64_t window = !objects || cap >= per_board ? max_objects : (cap - 4) / kRec;
    const int64_t chunk = !objects ? std::min<int64_t>(kSearchChunk, cap / 4)
                                   : std::max<int64_t>(1, std::min<int64_t>(kSearchChunk, cap / (4 + kRec * window)));
    if (objects && chunk * window * kRec > b->objects_host_bytes) {
        if (b->objects_host) BHIPCHK(b, hipHostFree(b->objects_host));
        b->objects_host = nullptr;
        b->objects_host_bytes = 0;
        BHIPCHK(b, hipHostMalloc(reinterpret_cast<void **>(&b->objects_host), (size_t)(chunk * window * kRec)));
        b->objects_host_bytes = chunk * window * kRec;
    }
    BatchObjectsParams op{};
    op.board_pitch = b->board_words;
    op.wd = b->wd;
    op.width = (int32_t)b->width;
    op.height = (int32_t)b->height;
    op.plane = b->topology == GOLHIP_TOPOLOGY_PLANE ? 1 : 0;
    op.reach = reach;
    op.max_objects = max_objects;
    op.window = (int32_t)window;
    for (int64_t i = 0; i < nboards; i += chunk) {
        const int64_t n = std::min<int64_t>(chunk, nboards - i);
        // the records first (8-byte aligned: the stage is), the counts behind them
        op.boards = base + i * b->board_words;
        op.objects = objects ? reinterpret_cast<ObjectRecord *>(b->search_stage) : nullptr;
        op.nobjects = reinterpret_cast<int32_t *>(b->search_stage + (objects ? n * window * kRec : 0));
        int64_t stored = 0;  // the records of the chunk's fullest board, cut at the cap
        for (int64_t first = 0; first == 0 || first < stored; first += window) {
            op.first = (int32_t)first;
            BHIPCHK(b, launch_batch_objects((int)n, op, b->stream));  // a missing kernel is an error
            if (first == 0) {
                BHIPCHK(b, hipMemcpyAsync(nobjects + i, op.nobjects, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost,
                                          b->stream));
                BHIPCHK(b, hipStreamSynchronize(b->stream));
                for (int64_t j = 0; j < n; ++j) stored = std::max<int64_t>(stored, std::min<int64_t>(nobjects[i + j], max_objects));
            }
            if (!objects || stored == 0) break;
            const int64_t cols = std::min(window, stored - first);  // per board, the widest row of this window
            BHIPCHK(b, hipMemcpy2DAsync(b->objects_host, (size_t)(cols * kRec), op.objects, (size_t)(window * kRec),
                                        (size_t)(cols * kRec), (size_t)n, hipMemcpyDeviceToHost, b->stream));
            BHIPCHK(b, hipStreamSynchronize(b->stream));  // the next launch rewrites the stage
            for (int64_t j = 0; j < n; ++j) {
                const int64_t m = std::min<int64_t>(std::min<int64_t>(nobjects[i + j], max_objects) - first, cols);
                if (m > 0)
                    std::memcpy(objects + (i + j) * max_objects + first, b->objects_host + j * cols * kRec, (size_t)(m * kRec));
            }
        }
    }
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    return GOLHIP_OK;
}

int golhip_batch_objects(golhip_batch_t b, int max_objects, int reach, int32_t *nobjects, golhip_object_t *objects) {
    if (!b) return GOLHIP_ERR_ARG;
    const int rc = objects_check(b, max_objects, reach);
    if (rc) return rc;
    if (!nobjects) return bfail(b, GOLHIP_ERR_ARG, "objects nobjects is null");
    BHIPCHK(b, hipSetDevice(b->device));
    return objects_boards(b, b->boards, b->nboards, max_objects, reach, nobjects, objects);
}

int golhip_batch_search_objects(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds, uint64_t seed0,
                                uint32_t density_q32, int64_t max_turns, const uint32_t *birth, const uint32_t *survive,
                                int max_objects, int reach, golhip_soup_t *out, int64_t *cycle_start, int64_t *ash_turn,
                                int32_t *nobjects, golhip_object_t *objects) {
    const SearchObjects so{max_objects, reach, ash_turn, nobjects, objects};
    return search_run(b, nsoups, seeds, seed0, density_q32, max_turns, birth, survive, out, cycle_start, true, nullptr,
                      &so);
}

int golhip_batch_set_topology(golhip_batch_t b, int topology) {
    if (!b) return GOLHIP_ERR_ARG;
    if (topology != GOLHIP_TOPOLOGY_TORUS && topology != GOLHIP_TOPOLOGY_PLANE)
        return bfail(b, GOLHIP_ERR_ARG, "topology %d: 0 (a torus) or 1 (a plane)", topology);
    if (topology == b->topology) return GOLHIP_OK;
    // the settle and period records describe the boards under one rule on one topology
    if (b->track && b->turn > 0)
        return bfail(b, GOLHIP_ERR_STATE, "settle tracking is on at turn %lld: the settle record holds on one topology, "
                     "change it at turn 0 (after a load)", (long long)b->turn);
    if (b->track_period && b->turn > 0)
        return bfail(b, GOLHIP_ERR_STATE, "period tracking is on at turn %lld: a repeat means a cycle on one topology "
                     "only, change it at turn 0 (after a load)", (long long)b->turn);
    b->topology = topology;
    return GOLHIP_OK;
}

int golhip_batch_get_topology(golhip_batch_t b, int *topology) {
    if (!b || !topology) return GOLHIP_ERR_ARG;
    *topology = b->topology;
    return GOLHIP_OK;
}

int golhip_batch_set_soup_box(golhip_batch_t b, int box_w, int box_h) {
    if (!b) return GOLHIP_ERR_ARG;
    const bool off = box_w == 0 && box_h == 0;
    if (!off && (box_w < 1 || box_w > b->width || box_h < 1 || box_h > b->height))
        return bfail(b, GOLHIP_ERR_ARG, "soup box %d x %d: 1..%lld by 1..%lld cells, or 0, 0 for the whole board", box_w,
                     box_h, (long long)b->width, (long long)b->height);
    b->box_w = box_w;
    b->box_h = box_h;
    return GOLHIP_OK;
}

int golhip_batch_get_soup_box(golhip_batch_t b, int *box_w, int *box_h) {
    if (!b || !box_w || !box_h) return GOLHIP_ERR_ARG;
    *box_w = b->box_w;
    *box_h = b->box_h;
    return GOLHIP_OK;
}

int golhip_batch_kernel(golhip_batch_t b, int *form) {
    if (!b || !form) return GOLHIP_ERR_ARG;
    *form = kernel_form(b);
    return GOLHIP_OK;
}

}  // extern "C"
