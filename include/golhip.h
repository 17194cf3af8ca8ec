/*
 * golhip.h -- C ABI of libgolhip, the MI355X (gfx950) Game-of-Life engine.
 *
 * libgolhip replaces the reference's per-turn compute path (Oliver-Cairns/distributed-gol):
 *
 *   reference (Go, net/rpc)                                   replaced by
 *   -------------------------------------------------------   ----------------------------------
 *   Broker.Publish(req, res)        broker/broker.go:157-180  golhip_step()  (res.World = next gen)
 *     publish: 4-strip fan-out      broker/broker.go:37-56    row strips over GPUs (golhip_create*)
 *     strip stitch + worldSave      broker/broker.go:168-175  device-resident board, halos by RCCL
 *   GolOP.Work(req, res)            server/server.go:77-107   gfx950 stencil kernel (k gens/launch)
 *     calculateNextState/updateCell server/server.go:21-75    bit-sliced B3/S23 (64 cells per uint64)
 *   calculateAliveCells             gol/distributor.go:153-166 golhip_alive_count / golhip_alive_cells
 *   CellFlipped diff                gol/distributor.go:53-59  golhip_flips
 *   readPgmImage / writePgmImage    gol/io.go:42-128          golhip_load_bytes / golhip_store_bytes
 *   Broker.CheckStates/Pause state  broker/broker.go:124-155  golhip_turn + the resident board
 *
 * Conventions (all functions):
 *   - return 0 (GOLHIP_OK) or a negative GOLHIP_ERR_* code; golhip_last_error(h) describes the
 *     last failure on that handle (the reference only prints RPC errors, gol/distributor.go:50-52;
 *     here every failure is reported, never silently ignored).
 *   - a handle is owned by ONE host thread; caller-owned host buffers are never retained.
 *   - cells are bytes: 0 = dead, any nonzero = alive on input (gol_test.go:119), 255 on output
 *     (server/server.go:37,46).  The board is a torus (server/server.go:58-69).
 *   - "the handle's rows" are [y0, y0+rows) of the global board (golhip_get_info): the whole board
 *     for golhip_create(), this rank's row strip for golhip_create_rank().
 *   - functions marked COLLECTIVE must be called by every rank of a golhip_create_rank() group.
 */
#ifndef GOLHIP_H
#define GOLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct golhip_engine *golhip_t;

#define GOLHIP_OK 0
#define GOLHIP_ERR_ARG (-1)   /* invalid argument (sizes, null pointers, k range) */
#define GOLHIP_ERR_HIP (-2)   /* HIP runtime error */
#define GOLHIP_ERR_OOM (-3)   /* device allocation failed */
#define GOLHIP_ERR_CAP (-4)   /* output capacity too small: *n holds the required count */
#define GOLHIP_ERR_RCCL (-5)  /* RCCL error */
#define GOLHIP_ERR_NODEV (-6) /* no gfx950 device / not enough devices */
#define GOLHIP_ERR_STATE (-7) /* call not valid in the current state (e.g. flips after k>1) */

#define GOLHIP_NCCL_ID_BYTES 128
#define GOLHIP_DENSITY_HALF 0x80000000u /* density_q32 for p = 0.5 (raw random bits) */

typedef struct {
    int64_t width;        /* logical board width  (Params.ImageWidth,  gol/gol.go:6-11) */
    int64_t height;       /* logical board height (Params.ImageHeight) */
    int64_t torus_width;  /* device torus width L = lcm(width, 128) (horizontal replication) */
    int64_t y0;           /* first global row held by this handle */
    int64_t rows;         /* rows held by this handle */
    int32_t rank;         /* first rank of this handle */
    int32_t world_size;   /* number of row strips (GPUs) the board is split over */
    int32_t nshards;      /* strips owned by this handle (ngpus for golhip_create) */
    int32_t k;            /* generations per stencil launch (temporal blocking depth) */
    int32_t halo_rows;    /* halo rows allocated per strip edge (>= k when world_size > 1) */
    int32_t band_rows;    /* rows per wave band in the stencil launch (0 = automatic) */
} golhip_info;

/* ---- library / devices ------------------------------------------------------------------ */
int golhip_version(void);                 /* e.g. 100 for 0.1.0 */
const char *golhip_strerror(int code);
int golhip_device_count(int *out);        /* visible HIP devices */
/* Pure host helper: the row strip of `rank` when `height` rows are split over world_size GPUs. */
int golhip_strip_bounds(int64_t height, int world_size, int rank, int64_t *y0, int64_t *rows);

/* One transfer of the halo exchange, in the order the engine issues it inside one RCCL group
 * (kind 0 = send, 1 = receive; rows relative to the strip's row 0, negative = top halo).
 * With world_size == 2 both neighbours are the same peer: RCCL matches the i-th send of a rank
 * to a peer with the i-th receive of that peer, which this order keeps consistent. */
typedef struct {
    int32_t kind;
    int32_t peer;
    int64_t row;
    int64_t nrows;
} golhip_xfer;
/* Pure host helper: the 4 transfers of `rank` for a k-row exchange (out[4]). */
int golhip_halo_plan(int64_t height, int world_size, int rank, int k, golhip_xfer *out);

/* ---- lifetime --------------------------------------------------------------------------- */
/* One process, `ngpus` devices (0..ngpus-1), one row strip each
 * (the on-node replacement of the broker + 4 servers, broker/broker.go:191-205), halos moved by
 * peer copies over xGMI. k = max generations per temporal-blocking stencil launch (1..32; the
 * whole-board kernel of golhip_set_board_kernel is not bounded by it). */
int golhip_create(int width, int height, int ngpus, int k, golhip_t *out);
/* One process, `nstrips` row strips placed on devices 0..ndevices-1 (strip s on device
 * s*ndevices/nstrips), halos by peer copies.  golhip_create(w, h, n, k) == create_strips(w, h, n, n, k);
 * nstrips > ndevices exercises the multi-strip path on fewer GPUs. */
int golhip_create_strips(int width, int height, int nstrips, int ndevices, int k, golhip_t *out);
/* One process per GPU: rank `rank` of `world_size`, on HIP device `device`. nccl_id: the
 * GOLHIP_NCCL_ID_BYTES produced by golhip_nccl_unique_id() on rank 0 (NULL if world_size == 1).
 * Test hook: with world_size == 1 and the environment variable GOLHIP_RING_SELF set (nonzero) the
 * board is a ring of ONE halo'd strip whose halos go through RCCL send/recv to itself (the
 * rank-mode path on a single GPU).
 * The communicator is non-blocking: a rank whose peers never join fails after the comm timeout.
 * GOLHIP_RING_SELF and GOLHIP_STAGE_BYTES (the transfer stage's size in bytes, read at create;
 * tests shrink it to force many row chunks) are the only environment variables the production
 * library reads (fault injection for the fail-fast tests is in the tuning library only). */
int golhip_nccl_unique_id(uint8_t *out /* GOLHIP_NCCL_ID_BYTES */);
int golhip_create_rank(int width, int height, int rank, int world_size, int device, int k,
                       const uint8_t *nccl_id, golhip_t *out);
/* The rank-mode engine with the caller's host transport in place of RCCL (the same strips,
 * launch plan, halo plan, interior/boundary overlap and count reduction; only the transport
 * differs).  Each K-block the engine copies its two send blocks of K rows to pinned host
 * buffers and calls exchange() with the 4 transfers of golhip_halo_plan in issue order
 * (bufs[i]: K * torus_width/8 bytes, a send's payload or a receive's destination; the i-th
 * send to a peer must match that peer's i-th receive from this rank); allreduce_u64 sums n
 * values over the ranks in place (per-turn counts, golhip_alive_count).  Both return 0 on
 * success; anything else fails the call with GOLHIP_ERR_RCCL.  For hosts whose ranks cannot
 * use RCCL peers -- e.g. several ranks sharing one GPU in a test, which RCCL refuses
 * ("Duplicate GPU"); the cgo host would hand its own transport here the same way.  `comm` is
 * copied; ctx must outlive the handle. */
typedef struct {
    void *ctx;
    int (*exchange)(void *ctx, const golhip_xfer *xfers, int n, void *const *bufs, size_t bytes);
    int (*allreduce_u64)(void *ctx, uint64_t *vals, size_t n);
} golhip_host_comm;
int golhip_create_rank_host(int width, int height, int rank, int world_size, int device, int k,
                            const golhip_host_comm *comm, golhip_t *out);
int golhip_destroy(golhip_t h);
const char *golhip_last_error(golhip_t h);  /* h == NULL: why the last create failed (this thread) */
int golhip_get_info(golhip_t h, golhip_info *out);

/* ---- board in / out (gol/io.go:42-128, util/cell.go) ------------------------------------- */
/* Load the handle's rows from 0/nonzero bytes (row y at cells + (y - y0) * row_stride). */
int golhip_load_bytes(golhip_t h, const uint8_t *cells, size_t row_stride);
/* Counter-based random board, regenerated on device (identical for any world_size):
 * width % 64 == 0; logical uint64 word i = y * width/64 + j:
 *   density_q32 == GOLHIP_DENSITY_HALF : word = splitmix64(seed + (i+1) * 0x9E3779B97F4A7C15)
 *   otherwise : cell c = y*width + x alive iff (uint32)splitmix64(seed + (c+1)*0x9E37..) < density_q32 */
int golhip_init_random(golhip_t h, uint64_t seed, uint32_t density_q32);
/* Store the handle's rows as 0/255 bytes (the PGM body, gol/io.go:76-81). */
int golhip_store_bytes(golhip_t h, uint8_t *out, size_t row_stride);
/* Packed little-endian uint64 rows of the handle's rows (width % 64 == 0): rows * width/64 words. */
int golhip_store_words(golhip_t h, uint64_t *out);
int golhip_load_words(golhip_t h, const uint64_t *in);

/* ---- windowed access: a rectangle of the board, and a density viewport ----------------------
 * The reference shows the world in an SDL window, one pixel per cell (sdl/loop.go, sdl/window.go),
 * and its `s` key writes the whole world as a PGM (gol/distributor.go:93-103).  At 65536^2 neither
 * can be used (nobody displays 65536^2 pixels; the PGM is 4 GiB), so these calls move only a window:
 * a rectangle of cells as bytes, out and in, and a viewport in which one pixel stands for a
 * scale x scale block of cells.  Their cost follows the window, not the board.
 *   - Coordinates are GLOBAL board coordinates.  x and y may be any int64 and are taken mod width /
 *     height; the rectangle wraps round the torus in both directions.  1 <= w <= width and
 *     1 <= hgt <= height.
 *   - The viewport: scale is a power of two in 1..1024, w * scale <= width and hgt * scale <= height
 *     (no cell is covered twice).
 *   - Anything else, a null buffer, row_stride < w or a mode outside 0..2 is GOLHIP_ERR_ARG: the
 *     board is untouched and golhip_last_error names the offending value.
 *   - All four synchronise the handle first, as golhip_store_bytes does (in rank mode within the
 *     comm timeout).  None allocates device memory: they stage through the transfer stage in chunks.
 *   - A handle that owns several strips (golhip_create, golhip_create_strips) serves each row from
 *     the strip that holds it; a viewport block that straddles two strips is the sum of their parts.
 *   - A handle that does NOT hold every row (rank mode, world_size > 1): the calls are not
 *     collective.  golhip_store_rect and golhip_view_counts write `out` in full, cells of rows the
 *     handle does not hold reading as dead, so the ranks' results combine by OR / by sum;
 *     golhip_load_rect ignores rows it does not hold (every rank passes the same rectangle);
 *     golhip_view returns GOLHIP_ERR_STATE (a partial count has no grey value: reduce the counts).
 *   - They do not depend on the rule (golhip_set_rule). */
#define GOLHIP_RECT_COPY 0 /* rectangle := cells */
#define GOLHIP_RECT_OR 1   /* rectangle |= cells */
#define GOLHIP_RECT_XOR 2  /* rectangle ^= cells */
/* Cells of the w x hgt rectangle whose top-left cell is (x, y), as 0/255 bytes
 * (out[j * row_stride + i] = cell (x + i, y + j)). */
int golhip_store_rect(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, uint8_t *out,
                      size_t row_stride);
/* Write 0/nonzero bytes into that rectangle of the RUNNING board (drop a pattern in): a change to
 * the board, not a new board, so the turn is kept.  What was derived from the old cells is dropped:
 * golhip_flips returns GOLHIP_ERR_STATE until the next step, and no stable slab is skipped on the
 * strength of flags from before the change (golhip_set_activity).  Captured graphs stay valid (the
 * same buffers and parity).  Only rows the handle owns are written; halo rows are exchanged again at
 * the start of the next step block, as after golhip_load_bytes. */
int golhip_load_rect(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, const uint8_t *cells,
                     size_t row_stride, int mode);
/* Viewport: pixel (i, j) of the w x hgt output covers the scale x scale block of cells whose
 * top-left cell is (x + i*scale, y + j*scale); out[j*w + i] = live cells in it. */
int golhip_view_counts(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, int scale,
                       uint32_t *out /* w*hgt, dense */);
/* The same as a grey image: grey = (count*255 + scale*scale - 1) / (scale*scale), i.e.
 * ceil(255 * count / scale^2): an empty block is 0, any live cell at least 1, a full block 255.
 * At scale 1 it equals golhip_store_rect. */
int golhip_view(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, int scale, uint8_t *out,
                size_t row_stride);

/* ---- checkpoint: the broker's paused state (broker/broker.go:124-155) ---------------------
 * The reference keeps worldSave/turn/size in the broker process between controller runs ('q'
 * sends Pause{P: true, Turn, Dimension}; the next controller's CheckStates resumes when the size
 * matches, gol/distributor.go:69-91).  Here that state is a file: the handle's rows as packed
 * bits (64-byte header: "GOLCKPT1", version 1, width, height, y0, rows, turn, row bytes; then
 * rows x ceil(width/8) bytes, LSB-first) and the completed turn, written atomically (tmp +
 * rename).  A rank-mode handle writes/loads its own strip (one file per rank).  The rule is not
 * part of the file: the caller restores it (golhip_set_rule). */
int golhip_checkpoint_save(golhip_t h, const char *path);
/* Restores the board and turn; GOLHIP_ERR_STATE if the file holds another board or strip. */
int golhip_checkpoint_load(golhip_t h, const char *path);
/* Pure host helper: the board size and turn a checkpoint holds (CheckStates' SameSize test). */
int golhip_checkpoint_info(const char *path, int64_t *width, int64_t *height, int64_t *turn);

/* ---- the rule ---------------------------------------------------------------------------- */
/* Life-like rules: outer-totalistic on the 8-cell Moore neighbourhood, written B<digits>/S<digits>.
 * In `birth`, bit n (0..8) means a dead cell with n live neighbours is born; in `survive`, bit n
 * means a live cell with n live neighbours stays alive.  A handle starts with the reference's rule
 * (calculateNextState, server/server.go:21-52): B3/S23, birth = 0x008, survive = 0x00C.
 *
 * Pure host helper: "B36/S23" (case-insensitive; digits 0-8, either list may be empty: "B2/S")
 * -> masks.  GOLHIP_ERR_ARG on anything else (digit 9, repeated digit, missing B or S part,
 * trailing text, NULL); golhip_last_error(NULL) then names the offending text. */
int golhip_parse_rule(const char *rule, uint32_t *birth, uint32_t *survive);
/* Set the handle's rule (golhip_set_rule = golhip_parse_rule + golhip_set_rule_masks; masks with
 * bits above 8: GOLHIP_ERR_ARG).  The board, the turn, flip tracking and every tuning setting are
 * kept; a change of rule synchronises the handle and drops what is cached per launch shape (captured
 * graphs, the stable-slab flags).  On failure the handle is untouched and golhip_last_error(h) names
 * the offending text.  In rank mode every rank sets the same rule.
 *   - B3/S23, defaulted or set explicitly, runs exactly the kernels and launch plan it always did.
 *   - Any other rule runs the rule-generic streaming kernel gol_rule on every launch of golhip_step,
 *     golhip_step_flips, golhip_step_flips_rows, flip tracking and per-turn counts, on single
 *     strips, golhip_create_strips and both rank modes: golhip_launch_kind* reports kind 5, with
 *     *param = 1 for a rule with a constant-folded kernel (the catalogue: HighLife B36/S23, Day &
 *     Night B3678/S34678, Seeds B2/S, Replicator B1357/S1357) and 0 for the table form, which serves
 *     every other rule and is slower.  Its launches are 8, 4, 2 or 1 generations deep: the largest
 *     that fits min(k, turns left).  The register slabs, gol_tile, the level split, the whole-board
 *     kernel, graph replays and stable-slab skipping are bypassed whatever golhip_set_board_kernel /
 *     golhip_set_activity / golhip_set_graphs say, and golhip_step_persistent returns
 *     GOLHIP_ERR_STATE before any device work.
 *   - B0 rules are allowed: the device torus has no dead padding (columns beyond `width` are
 *     replicas of the board, rows wrap mod height).
 *   - A checkpoint (GOLCKPT1) does not record the rule: the caller sets it again after
 *     golhip_checkpoint_load on a new handle. */
int golhip_set_rule(golhip_t h, const char *rule);
int golhip_set_rule_masks(golhip_t h, uint32_t birth, uint32_t survive);
int golhip_get_rule(golhip_t h, uint32_t *birth, uint32_t *survive);

/* ---- the hot path ------------------------------------------------------------------------ */
/* Advance `turns` generations (Broker.Publish called `turns` times, gol/distributor.go:48-49).
 * alive_per_turn (nullable, len turns): alive cells after each completed turn, counted inside the
 * stencil launch (the AliveCellsCount/TurnComplete source, gol/distributor.go:168-191).
 * COLLECTIVE when alive_per_turn != NULL or world_size > 1.  Asynchronous when alive_per_turn
 * is NULL (use golhip_sync to wait). */
int golhip_step(golhip_t h, int64_t turns, uint64_t *alive_per_turn);
/* Pure host helper: the launch depths golhip_step(turns) runs on a width x height board held as
 * `strips` row strips with maximum depth k (the reference has no such split: it runs one turn per
 * Broker.Publish, gol/distributor.go:48-49).  depths[i] > 0: one stencil launch of that many
 * generations; < 0: one captured graph replay of -depths[i] generations (small boards).  Large
 * boards run the depth <= k with the highest measured rate in bulk and split the last ones by a
 * modelled-time plan (e.g. 20 turns at 65536^2 -> 12 + 8, not 16 + 4).  Row strips are planned
 * from the largest strip, ceil(height / strips) rows, so every rank of a rank-mode board runs this
 * same sequence (each launch exchanges K-row halos) even when the strips differ by a row.
 * *n = number of entries; depths may be NULL to size the array; GOLHIP_ERR_CAP if cap is too
 * small.  It takes no handle and always describes the B3/S23 plan (another rule runs 8 / 4 / 2 / 1
 * deep launches of gol_rule, see golhip_set_rule). */
int golhip_launch_plan(int64_t width, int64_t height, int strips, int k, int64_t turns,
                       int32_t *depths, size_t cap, size_t *n);
/* Alive cells of the whole board (COLLECTIVE: sums over ranks). */
int golhip_alive_count(golhip_t h, uint64_t *out);
/* Alive cells of the handle's rows as (x, y) int32 pairs, row-major (gol/distributor.go:153-166).
 * If the count exceeds cap, returns GOLHIP_ERR_CAP with *n = required count. */
int golhip_alive_cells(golhip_t h, int32_t *xy, size_t cap, size_t *n);
/* Cells that changed in the last generation (gol/distributor.go:53-59), (x, y) pairs, row-major.
 * Valid after any golhip_step when flips tracking is on (the step's last launch writes them
 * beside its output), or after a step whose last launch advanced 1 generation; GOLHIP_ERR_STATE
 * otherwise. */
int golhip_flips(golhip_t h, int32_t *xy, size_t cap, size_t *n);
/* Flips tracking: every golhip_step keeps the flips of its last generation (one extra store per
 * row in its last launch), so golhip_flips is valid after a K-deep step. */
int golhip_track_flips(golhip_t h, int enable);
/* Per-turn CellFlipped for event consumers (the reference's per-turn diff, gol/distributor.go:
 * 53-59, and TurnComplete, :180-184): advance `turns` generations (<= golhip_flips_ring_capacity)
 * keeping each turn's flips in a device ring, then return them in ONE extraction: xy = every
 * turn's flipped cells, turn by turn, row-major within a turn; flips_per_turn[t] (nullable, len
 * turns) = cells flipped by turn t; alive_per_turn as in golhip_step.  If cap is too small the
 * turns are still advanced, GOLHIP_ERR_CAP is returned with *n = the required count and
 * golhip_flips_fetch returns them.  COLLECTIVE like golhip_step. */
int golhip_step_flips(golhip_t h, int64_t turns, int32_t *xy, size_t cap, size_t *n,
                      uint64_t *flips_per_turn, uint64_t *alive_per_turn);
int golhip_flips_ring_capacity(golhip_t h, int64_t *out);
int golhip_flips_fetch(golhip_t h, int32_t *xy, size_t cap, size_t *n, uint64_t *flips_per_turn);
/* The same per-turn flips (gol/distributor.go:53-59) in a compact form for consumers that take
 * rows: x[i] (uint16, width <= 65536) in the same turn-major, row-major order, and
 * row_offsets[t * rows + y] = the index in x of the first flip of turn t on row y of this
 * handle's strip (rows = golhip_info.rows; row y is board row golhip_info.y0 + y),
 * row_offsets[turns * rows] = *n (turns * rows + 1 entries, always written).  2 bytes per flip
 * instead of an 8-byte (x, y) pair: the list's transfer is what bounds golhip_step_flips on boards
 * with many flips.  One strip per handle (GOLHIP_ERR_STATE otherwise).  A too-small cap returns
 * GOLHIP_ERR_CAP with *n and row_offsets set; golhip_flips_fetch_rows returns the cells then.
 * COLLECTIVE like golhip_step. */
int golhip_step_flips_rows(golhip_t h, int64_t turns, uint16_t *x, size_t cap, size_t *n,
                           uint64_t *row_offsets, uint64_t *alive_per_turn);
int golhip_flips_fetch_rows(golhip_t h, uint16_t *x, size_t cap, size_t *n, uint64_t *row_offsets);
/* Completed turns since the last load (the broker's `turn`, broker/broker.go:140). */
int golhip_turn(golhip_t h, int64_t *out);
int golhip_set_turn(golhip_t h, int64_t turn);

/* ---- tuning / measurement ---------------------------------------------------------------- */
int golhip_set_k(golhip_t h, int k);                 /* 1..32, <= halo_rows when world_size > 1 */
/* k is the MAXIMUM launch depth: long runs use the depth <= k with the highest measured rate
 * (golhip_launch_plan).  fixed != 0: every bulk launch is exactly k deep (depth sweeps). */
int golhip_set_fixed_k(golhip_t h, int fixed);
int golhip_set_band_rows(golhip_t h, int band_rows); /* 0 = automatic */
/* Graded bands (tuning): the streaming launch's rows end in `bands` bands of `rows` rows each
 * instead of full-height ones (0, 0 = uniform bands). */
int golhip_set_tail_bands(golhip_t h, int bands, int rows);
/* Which kernel a k-deep launch on this handle's first strip runs: *kind = 0 the streaming kernel
 * (gol_stencil, gol_step1 at k = 1), 1 the level-split kernel (*param = waves per band), 2 the
 * register-tile kernel gol_tile (*param = tile height T), 3 the register-slab kernel gol_slab
 * (*param = [10000 * row chains +] 100 * waves + rows per wave), 4 the whole-board kernel gol_board
 * (*param = 100 * waves + rows per segment; golhip_set_board_kernel), 5 the rule-generic streaming
 * kernel gol_rule of every rule but B3/S23 (*param = 1 constant-folded, 0 table form; golhip_set_rule).
 * Introspection for tests and the
 * bench line.  golhip_launch_kind describes a launch without per-generation counts,
 * golhip_launch_kind_counts one with (counting != 0) or without them: small boards pick a
 * different slab shape when counting. */
int golhip_launch_kind(golhip_t h, int k, int *kind, int *param);
int golhip_launch_kind_counts(golhip_t h, int k, int counting, int *kind, int *param);
/* Captured-graph replay of step blocks on single-strip small boards: -1 automatic (boards whose
 * launches are short), 0 never, 1 whenever the launch plan allows (tests, tuning). */
int golhip_set_graphs(golhip_t h, int mode);
/* Generations of per-turn counts summed per finalize launch (default 4096, minimum 128; tests
 * shrink it to exercise the flushes).  Synchronises the handle. */
int golhip_set_count_window(golhip_t h, int generations);
/* Deadline (ms) of every host wait on work behind an RCCL transfer in rank mode -- the
 * communicator's set-up at create, a halo exchange, the count all-reduce, a sync -- plus 10x the
 * modelled time of the stencil work queued since the last sync.  When it passes (or RCCL reports an
 * asynchronous error) the call returns GOLHIP_ERR_RCCL, with golhip_last_error naming the rank,
 * the pending operation, its peers, K and its byte count; the handle then only accepts
 * golhip_comm_abort / golhip_destroy.  A communicator whose set-up failed is aborted (nothing of
 * it is on the device); after set-up it is left in place until golhip_comm_abort or golhip_destroy
 * (which aborts a failed communicator, then drains the streams within the timeout) or the end of
 * the process.  h == NULL sets the default of later creates (120000).
 * The reference has no such bound: a dead server stalls Broker.Publish (broker/broker.go:58-84). */
int golhip_set_comm_timeout(golhip_t h, int64_t ms);
/* After GOLHIP_ERR_RCCL on a rank-mode handle: ncclCommAbort its communicator (RCCL aborts the
 * operations of it still running on the device, so a receive whose send never comes stops
 * spinning), after which golhip_destroy can drain the handle's streams and free its memory.
 * GOLHIP_ERR_STATE if the communicator has not failed. */
int golhip_comm_abort(golhip_t h);
int golhip_sync(golhip_t h);                         /* wait for all queued device work */
/* The whole-board kernel: a single-strip board of 128, 256 or 512 torus cells per row (any width up
 * to 512 whose lcm with 128 is one of them: the reference's 16/64/128/256/512 sizes) and 4 W R rows
 * (4 ... 512) runs in ONE workgroup holding the whole torus in registers, every golhip_step call as
 * one launch per 4096 generations: no temporal-blocking trapezoid, no halo lanes, no launch
 * boundary inside a call.  Its launches are therefore NOT bounded by the handle's k (the depth of
 * the temporal-blocking stencil launches; golhip_launch_plan lists them as up to 4096 deep), and
 * golhip_set_fixed_k(h, 1) turns it off (a depth sweep measures the k-deep stencil launches).  enable = -1 (default): boards of at most 256 rows (one CU does the
 * board's whole VALU work per generation: faster than the multi-workgroup slabs up to 256 rows,
 * slower at 512), 1: every board it fits, 0: never (A/B).  golhip_launch_kind reports it as
 * kind 4 (*param = 100 * waves + rows per segment).  GOLHIP_ERR_ARG outside -1 .. 1. */
int golhip_set_board_kernel(golhip_t h, int enable);
/* golhip_step with per-turn counts (alive_per_turn non-null) as ONE launch per count window of a
 * persistent slab kernel (gol_slabq): each slab waits for its 3 x 3 neighbourhood of slabs
 * through device counters (golhip_set_persistent_handoff) instead of for a launch boundary every 16
 * generations; the same board and counts as golhip_step (a tail under 16 turns runs through it).
 * Opt-in, for single-strip boards whose counting launch is a gol_slab2 12x7 / 16x6 / 12x8 / 16x4 slab
 * with at most one slab per CU (configs[1], configs[4]; GOLHIP_ERR_STATE otherwise), a handle with
 * k >= 16 and flip tracking off (golhip_track_flips: GOLHIP_ERR_STATE, use golhip_step).  Its
 * progress needs every slab resident at once: the call refuses with GOLHIP_ERR_STATE, before any
 * device work, when the occupancy query does not put the whole grid on the device or the slabs
 * exceed golhip_set_persistent_limit.  If a slab still waits over 200 ms (another process took
 * CUs) the call restores the board and turn it started from and returns GOLHIP_ERR_STATE: a failed
 * call never leaves the board half advanced (the reference's Publish gate never leaves the world
 * half-written either, broker/broker.go:109-120). */
int golhip_step_persistent(golhip_t h, int64_t turns, uint64_t *alive_per_turn);
/* The persistent slab's neighbour hand-off.  GOLHIP_HANDOFF_FENCED (default): agent-scope release /
 * acquire fences around each slab's block counter -- the memory model's own guarantee, ~2.6 us per
 * 16-generation block.  GOLHIP_HANDOFF_SC1: write-through (`sc1`) board stores drained before the
 * counter store and `sc1` loads, no fences -- the hand-off measured valid on gfx950 / ROCm 7.2 but not
 * guaranteed by the architecture documents; faster (configs[4] 0.64 vs 0.81 us/turn).  Opt-in. */
#define GOLHIP_HANDOFF_FENCED 0
#define GOLHIP_HANDOFF_SC1 1
int golhip_set_persistent_handoff(golhip_t h, int mode);
/* The CUs the caller owns for golhip_step_persistent: at most max_groups slabs (one workgroup per
 * CU each) may be assumed resident at once -- for a process sharing the GPU with other work (a
 * second engine, a CU-masked stream, another process).  0 (default): the whole device. */
int golhip_set_persistent_limit(golhip_t h, int max_groups);
/* Stable-slab skipping: the register-slab launches of single-strip boards skip every slab whose
 * neighbourhood did not change in the previous launch's last generation -- Life's radius-1 rule
 * keeps such a slab fixed for the launch's K generations -- copying it once and counting its cached
 * alive cells for each generation.  Results are identical either way.  enable = -1 (default):
 * boards with more slabs than CUs (with one slab per CU a launch lasts as long as its slowest
 * computed slab, so skipping saves nothing there; sparse 16384^2 runs 1.7x faster, dense boards
 * pay ~8 % for the flags), 1: every eligible launch, 0: never (A/B).  GOLHIP_ERR_ARG outside
 * -1 .. 1. */
int golhip_set_activity(golhip_t h, int enable);
/* Slab launches computed / skipped on this handle since it was created (stable-slab skipping). */
int golhip_activity_stats(golhip_t h, int64_t *computed, int64_t *skipped);
/* HIP-event timing of golhip_step calls on the handle's first strip (one event pair per call
 * around its back-to-back stencil launches); kernel_time reports the summed span, the number of
 * stencil launch blocks and generations. */
int golhip_timing(golhip_t h, int enable);
int golhip_kernel_time(golhip_t h, double *total_ms, int64_t *launches, int64_t *generations);
/* With timing on, on a board held as halo'd row strips (rank mode): the summed time the first
 * strip's compute stream waited, after each block's interior launch, for that block's two boundary
 * bands -- which wait for the halo exchange -- and the number of such blocks.  The part of a
 * rank's time its neighbours and the transport cost it (the N > 1 bench line's per-rank data). */
int golhip_edge_wait(golhip_t h, double *total_ms, int64_t *blocks);

/* ---- batched small boards: many independent tori in one launch -------------------------------
 * The reference runs one world per broker (broker/broker.go:157-180).  A soup search, a seed or
 * density sweep or a census of what boards settle to runs thousands of small ones: a batch holds
 * `nboards` independent tori of one size on one device and advances all of them per launch, one
 * workgroup per board (gol_batch), with an optional per-board per-turn population history and
 * on-device detection of the turn at which each board became periodic with period <= 2.
 *   - Sizes: exactly those of the whole-board kernel (golhip_set_board_kernel): lcm(width, 128) of
 *     128, 256 or 512 cells (the reference's 16/64/128/256/512 widths) and 4, 8, 16, ..., 512 rows.
 *     Anything else, or nboards < 1, is GOLHIP_ERR_ARG with the offending value in
 *     golhip_batch_last_error(NULL) and no handle; a failed allocation is GOLHIP_ERR_OOM and frees
 *     what it had.  One device per handle: several GPUs are several handles.
 *   - The rule is B3/S23 unless one is set: golhip_batch_set_rule and the block below it.
 *   - Board i of a load or store sits at cells + (i - first) * board_stride + y * row_stride; input
 *     0 / nonzero, output 0 / 255.  No call but create, the first golhip_batch_track_settle(b, 1), the
 *     first golhip_batch_track_period(b, 1) (a second boards-sized buffer, the snapshots, and one
 *     int64 per board), the first golhip_batch_set_rules and the first golhip_batch_search or
 *     golhip_batch_search_exact (one chunk's seeds, rule pairs, records and cycle starts: 3.5 MiB)
 *     and the first golhip_batch_census (the pattern table: 66 KiB)
 *     allocates device memory: bytes, seeds, rules, counts, history and the census's results go
 *     through a transfer stage in chunks.  One more call allocates: the first
 *     golhip_batch_search_census (one chunk's ash boards, at most 64 MiB, and their turns, 512 KiB;
 *     the search buffers and the pattern table too if no earlier call has).  And the objects calls
 *     (golhip_batch_objects, golhip_batch_search_objects): the stage their results come back through
 *     and pinned host memory of its size, each at most 64 MiB, and what golhip_batch_search_census
 *     allocates for the search.
 *   - A batch has ONE turn counter.  Any golhip_batch_load_bytes, even of part of the batch, and any
 *     golhip_batch_init_random set it to 0 and clear every settle and period record: a batch is filled, then run.
 *   - golhip_batch_init_random: board i is bit for bit what golhip_init_random(seed_i, density_q32)
 *     gives a single engine of that size, seed_i = seeds ? seeds[i] : seed0 + i (width % 64 == 0).
 *   - golhip_batch_step runs `turns` generations of every board and returns when they are done.
 *     history (nullable): history[i * board_stride + j] = alive cells of board i after the j-th turn
 *     of this call (board_stride >= turns, in uint32 units).  turns == 0 is a no-op.
 *   - Settling: with tracking on, settled[i] is the smallest absolute turn t >= 2 with
 *     board_i(t) == board_i(t - 2), or -1 while no such turn has been run; once set it never changes,
 *     and it does not depend on how the turns were cut into calls.  Tracking starts at turn 0:
 *     enabling it after turns have run is GOLHIP_ERR_STATE, golhip_batch_settled without it too.
 *   - Periods (golhip_batch_track_period / golhip_batch_periods): per-board cycle detection on the
 *     device, Brent's scheme with snapshots at turns 2^j - 1, for whatever rule or rules the batch
 *     runs.  For t >= 1 let s(t) = 2^floor(log2 t) - 1 (0 for t = 1, 1 for t = 2..3, 3 for t = 4..7,
 *     7 for t = 8..15, ...).  Board i repeats at turn t when board_i(t) == board_i(s(t)) over the
 *     whole torus; repeat_turn[i] is the smallest such t among the turns run so far and period[i] =
 *     repeat_turn[i] - s(repeat_turn[i]); both are -1 until a repeat has been run.  The rule is
 *     deterministic, so period[i] is exactly the period p of the cycle the board has entered, not
 *     a multiple of it: offsets inside a window only run up to the window's length, so the first
 *     match has offset p.  With m the first turn inside the cycle, the repeat is found at t =
 *     2^j - 1 + p for the first j with 2^j - 1 >= m and 2^j >= p: under 2 max(m + 1, p) + p turns.
 *     An empty or still-life board is (1, 1), a lone blinker (3, 2), a lone glider on a 16 x 16
 *     torus (p = 64) is (127, 64).  The records depend on the boards and the rule only: not on the
 *     sizes of the step calls, the launch depths, history on or off or GOLHIP_STAGE_BYTES.
 *     Enabling is legal at turn 0 only (GOLHIP_ERR_STATE otherwise): board(0) is the first
 *     snapshot.  golhip_batch_periods with tracking off is GOLHIP_ERR_STATE; either output may be
 *     NULL.  Period and settle tracking exclude each other: enabling one while the other is on is
 *     GOLHIP_ERR_STATE (switch the other off first).  They agree where both speak: a board with
 *     period <= 2 has settled = m + 2.  With period tracking on every rule form, B3/S23 included,
 *     launches gol_batch_period; golhip_batch_kernel still reports the rule form. */
typedef struct golhip_batch *golhip_batch_t;
int golhip_batch_create(int width, int height, int nboards, int device, golhip_batch_t *out);
int golhip_batch_destroy(golhip_batch_t b);
const char *golhip_batch_last_error(golhip_batch_t b); /* NULL: why the last create failed (this thread) */
int golhip_batch_load_bytes(golhip_batch_t b, int first, int n, const uint8_t *cells, size_t row_stride,
                            size_t board_stride);
int golhip_batch_store_bytes(golhip_batch_t b, int first, int n, uint8_t *out, size_t row_stride,
                             size_t board_stride);
int golhip_batch_init_random(golhip_batch_t b, const uint64_t *seeds /* nboards, or NULL */, uint64_t seed0,
                             uint32_t density_q32);
int golhip_batch_step(golhip_batch_t b, int64_t turns, uint32_t *history, size_t board_stride);
int golhip_batch_alive_counts(golhip_batch_t b, uint32_t *out /* nboards */);
int golhip_batch_track_settle(golhip_batch_t b, int enable);
int golhip_batch_settled(golhip_batch_t b, int64_t *out /* nboards */);
int golhip_batch_track_period(golhip_batch_t b, int enable);
int golhip_batch_periods(golhip_batch_t b, int64_t *repeat_turn /* nboards, or NULL */,
                         int64_t *period /* nboards, or NULL */);
int golhip_batch_turn(golhip_batch_t b, int64_t *out);
/* Life-like rules on a batch: one rule for all boards (golhip_batch_set_rule = golhip_parse_rule +
 * golhip_batch_set_rule_masks), or one per board (golhip_batch_set_rules: nboards birth masks and
 * nboards survive masks; both NULL: back to the uniform rule, which per-board rules do not change).
 * Masks as in golhip_set_rule.  A batch starts at B3/S23.
 *   - A uniform B3/S23, defaulted or set explicitly, launches gol_batch exactly as it always did.
 *     Any other rule launches gol_batch_rule -- the same geometry, history, settling and in-place
 *     update under the rule: a uniform catalogue rule (HighLife B36/S23, Day & Night B3678/S34678,
 *     Seeds B2/S, Replicator B1357/S1357) constant-folded, every other uniform rule in the table
 *     form, which is slower.  Per-board rules ALWAYS run the table form, also when they happen to
 *     be B3/S23 or catalogue rules.  golhip_batch_kernel: what the next step launches, *form = 0
 *     gol_batch, 1 constant-folded, 2 table, 3 table with per-board rules.
 *   - Setting a rule keeps the boards, the turn, the history behaviour and the settle and period switches;
 *     golhip_batch_load_bytes and golhip_batch_init_random do not touch the rule.
 *   - A mask with bits above 8 is GOLHIP_ERR_ARG; in a per-board array golhip_batch_last_error(b)
 *     names the board index and the mask.  A bad rule text is GOLHIP_ERR_ARG naming the text.  The
 *     handle is untouched either way.
 *   - The settle record and the period record are records of one rule: with either tracking on
 *     and turn > 0 any change of rule is GOLHIP_ERR_STATE (setting the rule the batch already has
 *     is no change).  Change it at turn 0, i.e. after a load.
 *   - golhip_batch_get_rule with per-board rules set is GOLHIP_ERR_STATE; golhip_batch_get_rules
 *     always answers (the uniform rule repeated when no per-board rules are set).
 *   - B0 rules are allowed, as on the engine: the torus has no dead padding.
 *   - The per-board rules live in device memory allocated by the first golhip_batch_set_rules and
 *     are uploaded through the transfer stage. */
int golhip_batch_set_rule(golhip_batch_t b, const char *rule);
int golhip_batch_set_rule_masks(golhip_batch_t b, uint32_t birth, uint32_t survive);
int golhip_batch_get_rule(golhip_batch_t b, uint32_t *birth, uint32_t *survive);
int golhip_batch_set_rules(golhip_batch_t b, const uint32_t *birth /* nboards */, const uint32_t *survive);
int golhip_batch_get_rules(golhip_batch_t b, uint32_t *birth /* nboards */, uint32_t *survive);
int golhip_batch_kernel(golhip_batch_t b, int *form);
/* The soup search: a soup is a seed.  One workgroup (gol_batch_search) generates the board of soup i
 * in registers -- bit for bit the board golhip_batch_init_random gives seed_i = seeds ? seeds[i] :
 * seed0 + i at density_q32 -- and runs it from generation 0, with the cycle detection of the block
 * above, until it repeats or max_turns have run; then the soup is retired and the workgroup ends.
 * No board memory is read or written: the footprint of a soup is its 32-byte record, and nsoups has
 * nothing to do with nboards.
 *   - out[i] depends on soup i's seed, the density, the board size, the rule, max_turns, the
 *     topology and the soup box (the block below) only: not on nsoups, the soup's position, the
 *     chunking or nboards.
 *   - repeat_turn and period are exactly what golhip_batch_init_random with that seed,
 *     golhip_batch_track_period, golhip_batch_step(max_turns) and golhip_batch_periods report; -1 and
 *     -1 when the soup has no repeat within max_turns.
 *   - stop_turn, the generations the soup ran, is a function of (repeat_turn, max_turns): max_turns
 *     when there is no repeat, else min(max_turns, 32 * ((repeat_turn - 1) / 32) + 40) (integer
 *     division): the kernel learns of a repeat once per 32 generations and every wave of the
 *     workgroup leaves 8 generations later, between repeat_turn + 8 and repeat_turn + 39.
 *   - population is the alive count of the soup at stop_turn; reserved is 0.
 *   - The handle gives the size, the device, the stream and the UNIFORM rule (golhip_batch_set_rule;
 *     B3/S23 runs LifeNext, a catalogue rule its constant-folded kernel, any other rule the table
 *     form).  The handle's per-board rules belong to its boards and do not apply to soups.  birth and
 *     survive, both given or both NULL, are nsoups masks each: soup i runs its own rule (the table
 *     form).  The search leaves the batch's boards, turn, settle and period records and switches
 *     exactly as they were.  To look at a soup, golhip_batch_init_random with its seed.
 *   - GOLHIP_ERR_ARG: width % 64 != 0 (as init_random); max_turns outside 1..2^20; nsoups < 0; a mask
 *     with bits above 8 (golhip_batch_last_error names the soup index and the mask); exactly one of
 *     birth and survive; out == NULL with nsoups > 0.  The handle and out are then untouched.
 *     nsoups == 0 is a no-op.
 *   - Soups are launched in chunks of at most 65536 soups and at most 2^44 cell updates (chunk *
 *     width * height * max_turns; never fewer than 1 soup), so that no launch runs long.  The first
 *     search allocates the device buffers of one chunk (seeds, rule pairs, records);
 *     golhip_batch_destroy frees them. */
typedef struct {
    int64_t repeat_turn, period, stop_turn;
    uint32_t population, reserved;
} golhip_soup_t;
int golhip_batch_search(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds /* nsoups, or NULL */,
                        uint64_t seed0, uint32_t density_q32, int64_t max_turns,
                        const uint32_t *birth /* nsoups, or NULL */, const uint32_t *survive,
                        golhip_soup_t *out /* nsoups */);
/* The exact search: golhip_batch_search plus, per soup, the turn at which it enters its cycle.
 * repeat_turn is the turn at which Brent's scheme NOTICES the repeat, always 2^j - 1 + period: every
 * soup whose ash forms between turn 1024 and turn 2047 reports 2048 (a still life), 2049 (blinkers)
 * and so on.  The quantity a soup search ranks on is the lifespan, the first turn of the cycle:
 *   - cycle_start[i], for a soup with a repeat within max_turns, is the least t >= 0 with
 *     board_i(t + period) == board_i(t), period being the record's (the cycle's minimal period);
 *     -1 for a soup without a repeat.
 *   - 0 <= cycle_start <= repeat_turn - period.
 *   - cycle_start + period <= repeat_turn <= max_turns: the exact pass never needs a generation
 *     beyond repeat_turn.
 *   - cycle_start == 0 exactly when board_i(0) is on the cycle (an empty board, a still life).
 *   - On a plane, in a soup box and under per-soup rules the definition holds word for word with the
 *     board stepped that way, as for every other field of the record.
 *   - out is byte for byte what golhip_batch_search writes for the same arguments; golhip_soup_t and
 *     golhip_batch_search are what they were.
 *   - Errors: golhip_batch_search's checks, texts and contract (the handle, out and cycle_start are
 *     then untouched); additionally cycle_start == NULL with nsoups > 0 is GOLHIP_ERR_ARG.
 *   - Chunks: golhip_batch_search's; cycle_start does not depend on the chunking, on nsoups or on the
 *     soup's position.  The chunk's device buffers hold 8 more bytes per soup (one chunk's seeds, rule
 *     pairs, records and cycle starts: 3.5 MiB), allocated with the search buffers by the first
 *     golhip_batch_search or golhip_batch_search_exact, whichever comes first, and freed by
 *     golhip_batch_destroy.
 *   - How: a second pass (gol_batch_cycle) behind each chunk's search launch, one workgroup per soup.
 *     With s = repeat_turn - period = 2^j - 1 the record gives cycle_start <= s and, if j > 0 and
 *     period <= 2^(j-1), cycle_start > 2^(j-1) - 1 (the previous snapshot would have matched inside
 *     its window otherwise); lo is that bound, else 0.  The pass re-seeds the soup, runs it lo
 *     generations, keeps a copy, runs it `period` more and then steps both in lockstep, comparing
 *     board(t + period) with board(t) from t = lo until they are equal: lo + period +
 *     2 (cycle_start - lo) generations plus at most 34 lockstep turns of detection slack, never
 *     above about 1.5 s + period.  Two forms: B3/S23's rule step for a uniform B3/S23, the table form
 *     for every other rule: a HighLife search runs its exact pass in the table form, and the
 *     results are the rule's, not the form's. */
int golhip_batch_search_exact(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds /* nsoups, or NULL */,
                              uint64_t seed0, uint32_t density_q32, int64_t max_turns,
                              const uint32_t *birth /* nsoups, or NULL */, const uint32_t *survive,
                              golhip_soup_t *out /* nsoups */, int64_t *cycle_start /* nsoups */);
/* Topology and the soup box: the standard search setting, a small random box in empty space on a
 * bounded grid whose outside is dead (Golly's :P64,64 where the torus is :T64,64).
 *   - A batch starts as a torus.  On GOLHIP_TOPOLOGY_PLANE the board is the same width x height
 *     cells, every neighbour outside the rectangle counts as dead and no cell outside is ever alive:
 *     under a B0 rule the cells inside are born as the rule says and the outside stays dead.  A
 *     glider that leaves the ash does not circle the board: it ends as a block at the border, so a
 *     lone glider on a 16 x 16 plane is (repeat_turn, period) = (64, 1) where the torus gives
 *     (127, 64), and a period above 2 on a plane always means an oscillator.
 *   - The plane runs every width and height a batch accepts, uniform and per-board rules, history,
 *     settle tracking, period tracking and golhip_batch_search.  Every definition above (settled,
 *     repeat_turn, period, stop_turn, population) holds word for word with "the board" stepped as a
 *     plane.
 *   - The plane has its own kernels (gol_plane_rule, gol_plane_period, gol_plane_search) in two
 *     forms: B3/S23's rule step for a uniform B3/S23 and the table form for everything else.  It has
 *     no constant-folded catalogue kernels: HighLife on a plane runs the table form.
 *     golhip_batch_kernel on a plane reports 0 for a uniform B3/S23, 2 for every other uniform rule
 *     and 3 for per-board rules.  A torus batch launches exactly what it launched before.
 *   - golhip_batch_set_topology keeps the boards, the turn, the rules and the switches.  It follows
 *     the rule-change contract: with settle or period tracking on and turn > 0 a change is
 *     GOLHIP_ERR_STATE (setting the current value is no change); change it at turn 0, i.e. after a
 *     load.  Any other value is GOLHIP_ERR_ARG and leaves the handle untouched.
 *     golhip_batch_load_bytes, golhip_batch_init_random and golhip_batch_store_bytes do not touch
 *     the topology.
 *   - The soup box: golhip_batch_set_soup_box(b, box_w, box_h) with 1 <= box_w <= width and 1 <=
 *     box_h <= height; (0, 0), the default, is the whole board; anything else is GOLHIP_ERR_ARG and
 *     leaves the handle untouched.  The box sits at x0 = (width - box_w) / 2, y0 = (height -
 *     box_h) / 2 (integer division).  The boxed soup of a seed is the full-board soup of that seed,
 *     for either density path, with every cell outside the box cleared: seeds keep their meaning.
 *     golhip_batch_init_random and golhip_batch_search both honour it, on either topology, so
 *     "search, then init_random with the seeds of interest" still shows the boards that were
 *     searched; golhip_batch_load_bytes ignores it.  A boxed search on the torus runs
 *     gol_plane_search with its seams switched off (B3/S23's rule step or the table form). */
#define GOLHIP_TOPOLOGY_TORUS 0
#define GOLHIP_TOPOLOGY_PLANE 1
int golhip_batch_set_topology(golhip_batch_t b, int topology);
int golhip_batch_get_topology(golhip_batch_t b, int *topology);
int golhip_batch_set_soup_box(golhip_batch_t b, int box_w, int box_h); /* 0, 0: the whole board (default) */
int golhip_batch_get_soup_box(golhip_batch_t b, int *box_w, int *box_h);
/* The census: what the boards hold, by pattern matching on the device.  A search record says when a
 * soup settled, with what period and how many cells; the census says into what: how many blocks,
 * beehives, blinkers, gliders ... are on each board, and how many live cells belong to none of the
 * listed objects.  A board with residue 0 is fully explained; anything else is worth a look.  One
 * workgroup per board (gol_batch_census) stages the board in LDS and matches every pattern at every
 * anchor, 32 anchors per lane.
 *   - Cells.  cell_i(x, y) is board i's cell.  On a torus the coordinates are taken mod width and mod
 *     height.  On a plane (golhip_batch_set_topology) a cell outside the rectangle is dead.
 *   - Match.  Pattern p matches board i at anchor (x, y) when cell_i(x + c, y + r) == alive_p(r, c) for
 *     every (r, c) in care_p.  Cells outside care_p are not looked at.
 *   - Anchors.  On a torus: 0 <= x < width, 0 <= y < height.  On a plane: -(w - 1) <= x <= width - 1
 *     and -(h - 1) <= y <= height - 1.  Every pattern has a live cell, so every match overlaps the
 *     board.  An object touching the plane's border, with its dead ring outside, is counted.
 *   - Counts.  counts[i * npat + p] is the number of matching anchors.  Overlapping matches each count.
 *   - Residue.  residue[i] is the number of live cells of board i not covered by any match.  A match
 *     (p, x, y) covers the cells (x + c, y + r) with alive_p(r, c) set, wrapped on a torus.  With
 *     npat == 0, residue is golhip_batch_alive_counts's result and counts is not touched.
 *   - Bad arguments.  The following are GOLHIP_ERR_ARG; the text names the pattern index and the
 *     offence, and the handle and outputs stay untouched: npat < 0 or npat > 256; patterns == NULL with
 *     npat > 0; both outputs NULL; w or h outside 1..32; w > width or h > height; a bit at column >= w,
 *     or in a row >= h; alive not a subset of care; a pattern without a live cell.
 *   - No side effects.  The call reads the boards as they are at the current turn.  It changes
 *     nothing: boards, turn, rule(s), settle, period and search records, switches, topology and box
 *     all stay as they were.  It is legal with tracking on or off and at any turn.  The rule plays no
 *     part.
 *   - Independence.  The result for board i depends on board i, the topology and the pattern list
 *     only.  It does not depend on nboards, on how boards are cut into launches, or on
 *     GOLHIP_STAGE_BYTES.  counts[.., p] does not depend on the other patterns.  residue does not
 *     depend on their order.
 *   - An oscillating ash is seen in the phase of the turn the batch is at: list an oscillator in
 *     every phase.  Either output may be NULL, not both; a NULL residue skips the cover work.
 *   - Boards go out in launches of at most 65536 boards; counts and residues come back through the
 *     transfer stage in chunks.  The pattern table lives in device memory (66 KiB) allocated by the
 *     first golhip_batch_census, the sixth and last allocating call of the list above, and freed by
 *     golhip_batch_destroy. */
typedef struct {
    int32_t  w, h;        /* 1..32 each */
    uint32_t alive[32];   /* row r, bit c set: cell (r, c) must be alive */
    uint32_t care[32];    /* row r, bit c set: cell (r, c) is looked at; alive is a subset of care */
} golhip_pattern_t;       /* 264 bytes */
int golhip_batch_census(golhip_batch_t b, const golhip_pattern_t *patterns, int npat,
                        uint32_t *counts  /* nboards * npat, or NULL */,
                        uint32_t *residue /* nboards, or NULL */);
/* The soup search with a census of each soup's ash, no boards kept: golhip_batch_search_exact plus, per
 * soup, the census of a board that lies on the soup's cycle.  The exact pass already holds such a
 * board in registers when it has found cycle_start; it stores that board into a chunk-sized buffer
 * and gol_batch_census runs over the buffer.  No second batch, no init_random, no stepping of every
 * board to the slowest soup's turn.
 *   - out is byte for byte what golhip_batch_search writes for the same arguments and cycle_start is
 *     what golhip_batch_search_exact writes; both are required, as is ash_turn.
 *   - The censused board of soup i is board_i(ash_turn[i]), the soup stepped ash_turn[i] generations
 *     from its seed under the batch's topology and soup box and the soup's rule.  For a soup with a
 *     repeat within max_turns, cycle_start <= ash_turn <= repeat_turn: the board is on the cycle and
 *     no generation beyond repeat_turn has run.  ash_turn is 0, the board the seeded soup, when
 *     repeat_turn == period (the soup is on its cycle and was noticed from the snapshot of turn 0:
 *     an empty board, a still life).  ash_turn is a function of the soup's record and cycle_start
 *     alone; it is NOT aligned to cycle_start's phase, so an oscillating ash is seen in the phase of
 *     turn ash_turn: list an oscillator in every phase.
 *   - The recipe that reproduces the censused board: a batch of the same size, topology and soup
 *     box, golhip_batch_init_random with the soup's seed, golhip_batch_step(ash_turn) under the
 *     soup's rule; golhip_batch_census of that board gives the same row.
 *   - counts[i * npat + p] and residue[i] are golhip_batch_census's, word for word, of that board
 *     under the batch's topology.  ash_cells[(i * height + y) * width + x] is its cell (x, y), 0 or 1.
 *     Each of counts, residue and ash_cells may be NULL, not all three; npat == 0 is allowed when
 *     counts is NULL, and residue is then the board's live cells.
 *   - A soup without a repeat within max_turns has ash_turn -1, a counts row of zeros, ash_cells all
 *     dead and residue = the record's population: the cells are alive and none is explained.
 *   - Errors: golhip_batch_search's checks, then golhip_batch_census's checks of npat and the patterns,
 *     in their words, all before any device work: GOLHIP_ERR_ARG, and the handle and every output
 *     stay untouched.  Additionally GOLHIP_ERR_ARG: counts, residue and ash_cells all NULL; counts
 *     with npat == 0; with nsoups > 0, out, cycle_start or ash_turn NULL.
 *   - Side effects are golhip_batch_search's: the batch's boards, turn, rules, records, switches,
 *     topology and box all stay.  The soup runs under the batch's uniform rule, or its own with birth
 *     and survive, as in golhip_batch_search_exact.
 *   - Independence.  Every output for soup i depends on what its record depends on and, for counts and
 *     residue, on the patterns; not on nsoups, the soup's position, the chunking or
 *     GOLHIP_STAGE_BYTES, nor on which of the optional outputs are asked for.
 *   - Chunks, in stream order: the search launch, the chunk's ash buffer zeroed, gol_batch_cycle with
 *     the buffer, the census over the buffer, the ash unpacked if ash_cells is set.  A chunk is
 *     golhip_batch_search's, capped so that the ash buffer stays at or below 64 MiB: 65536 soups of
 *     64 x 64, 2048 of 512 x 512.  The buffer is allocated by the first golhip_batch_search_census
 *     and freed by golhip_batch_destroy. */
int golhip_batch_search_census(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds /* nsoups, or NULL */,
                               uint64_t seed0, uint32_t density_q32, int64_t max_turns,
                               const uint32_t *birth /* nsoups, or NULL */, const uint32_t *survive,
                               const golhip_pattern_t *patterns, int npat,
                               golhip_soup_t *out /* nsoups */, int64_t *cycle_start /* nsoups */,
                               int64_t *ash_turn /* nsoups */,
                               uint32_t *counts  /* nsoups * npat, or NULL */,
                               uint32_t *residue /* nsoups, or NULL */,
                               uint8_t *ash_cells /* nsoups * height * width, or NULL */);
/* The objects: every cluster of live cells of every board, found and hashed on the device.  The census
 * counts the patterns of a list and says how many live cells the list does not explain; this call
 * needs no list.  For every board it returns the clusters of live cells, each with a position, an
 * extent, a population and a 64-bit shape hash that is the same for every translation, rotation and
 * reflection of the shape: one tally over the hashes of a million boards names everything that
 * occurred, listed or not.  One workgroup per board (gol_batch_objects) floods one cluster after the
 * other in LDS.
 *
 * Cluster.
 *   - reach is 1 or 2.
 *   - Two live cells of a board are linked when their Chebyshev distance is at most reach.  On a torus
 *     the distance is taken mod width and mod height.  On a plane it is taken in the rectangle.
 *   - A cluster is a connected component of that relation.
 *   - reach 1 gives 8-connected islands.
 *   - reach 2 joins cells whose neighbourhoods share a cell.  Two clusters then cannot influence each
 *     other in the next generation.  It keeps an aircraft carrier or a pulsar in one piece.
 * Order.  The clusters of a board are numbered by their first cell in row-major order: smallest y,
 * then smallest x.
 * Extent, per axis.
 *   - Take the cluster's occupancy along the axis: the columns, or rows, that hold one of its cells.
 *   - On a plane, x0 is the smallest occupied column and w is the span to the largest.
 *   - On a torus the occupancy is cyclic.  A connected cluster has at most one cyclic run of empty
 *     columns of length >= reach.
 *       - If that run exists, x0 is the column just after it, and w is the cyclic span from x0 to the
 *         last occupied column.
 *       - If it does not exist, the cluster winds round the torus on that axis: x0 = 0, w = width, and
 *         flag WINDS_X is set.  A single cell on a torus of width <= reach winds by this rule.
 *   - y0, h and WINDS_Y are defined the same way.
 *   - A cell's place in the cluster is dx = (x - x0) mod width, dy = (y - y0) mod height.
 * Hash.
 *   - mix(v) is the splitmix64 finaliser on 64-bit unsigned values:
 *       z = v + 0x9E3779B97F4A7C15
 *       z = (z ^ z>>30) * 0xBF58476D1CE4E5B9
 *       z = (z ^ z>>27) * 0x94D049BB133111EB
 *       result z ^ z>>31
 *   - The eight orientations k = 0..7 map (dx, dy) in a w x h box to (u, v) in an ow x oh box:
 *       k   u        v        ow x oh
 *       0   dx       dy       w x h
 *       1   w-1-dx   dy       w x h
 *       2   dx       h-1-dy   w x h
 *       3   w-1-dx   h-1-dy   w x h
 *       4   dy       dx       h x w
 *       5   h-1-dy   dx       h x w
 *       6   dy       w-1-dx   h x w
 *       7   h-1-dy   w-1-dx   h x w
 *   - H_k = (the sum over the cluster's cells of mix(v<<16 | u), mod 2^64) XOR mix(1<<32 | oh<<16 | ow).
 *   - hash is the smallest H_k as an unsigned number.
 *   - The sum does not depend on the order of the cells, so it can be reduced any way.
 *   - A cluster that does not wind has the same hash wherever it lies and however it is turned.
 *   - A winding cluster's hash depends on its position along the winding axis: its place is taken from
 *     column (row) 0, so the same shape moved along that axis hashes differently.
 * Record.  golhip_object_t is 32 bytes: int32 x, y, w, h; int32 population; uint32 flags; uint64 hash.
 *   - Flag bit 0 is WINDS_X.  Bit 1 is WINDS_Y.
 *   - Bit 2 is AT_BORDER.  It is set only on a plane, when a cell of the cluster is in row 0, row
 *     height - 1, column 0 or column width - 1.  A glider dying at the edge has it.
 *
 * golhip_batch_objects(b, max_objects, reach, nobjects, objects):
 *   - nobjects[i] is board i's total number of clusters, also when it exceeds max_objects.
 *   - objects holds max_objects records per board.  The first min(nobjects[i], max_objects) records
 *     of board i are written, at objects[i * max_objects ..], in the order above.  The rest are left
 *     untouched.  objects may be NULL, for the counts alone.
 *   - Bad arguments.  max_objects outside 1..4096, reach other than 1 or 2 and nobjects == NULL are
 *     GOLHIP_ERR_ARG; the text names the argument, all checks come before any device work, and the
 *     handle and outputs stay untouched.
 *   - No side effects.  The call reads the boards as they are at the current turn.  It changes
 *     nothing: boards, turn, rule(s), settle, period and search records, switches, topology and box
 *     all stay as they were.  It is legal with tracking on or off and at any turn.  The rule plays no
 *     part.
 *   - Independence.  The result for board i depends on board i, the topology and reach only.  It does
 *     not depend on nboards, on the board's position, on how boards are cut into launches, on
 *     GOLHIP_STAGE_BYTES or on max_objects: the cap only cuts the list.
 *   - Boards go out in launches of at most 65536 boards.  Counts and records come back in chunks
 *     through the stage golhip_batch_search_census uses (at most 64 MiB, capped by GOLHIP_STAGE_BYTES
 *     but never below one count and one record) and, the records, through pinned host memory of the
 *     same size; a stage that does not hold a board's max_objects records takes the board's records
 *     in several launches.  Both are allocated by the first call that needs them and freed by
 *     golhip_batch_destroy. */
#define GOLHIP_OBJECT_WINDS_X   1u
#define GOLHIP_OBJECT_WINDS_Y   2u
#define GOLHIP_OBJECT_AT_BORDER 4u
typedef struct {
    int32_t  x, y, w, h;   /* x0, y0 and the extent */
    int32_t  population;
    uint32_t flags;        /* GOLHIP_OBJECT_* */
    uint64_t hash;
} golhip_object_t;         /* 32 bytes */
int golhip_batch_objects(golhip_batch_t b, int max_objects /* 1..4096 */, int reach /* 1 or 2 */,
                         int32_t *nobjects /* nboards */,
                         golhip_object_t *objects /* nboards * max_objects, or NULL */);
/* The soup search with the objects of each soup's ash, no boards kept: golhip_batch_search_census with
 * golhip_batch_objects in the census's place.  The same chunks, ash buffer and ash_turn; out,
 * cycle_start and ash_turn are byte for byte golhip_batch_search_census's, and all three are required
 * with nsoups > 0, as is nobjects.  nobjects[i] and objects[i * max_objects ..] are
 * golhip_batch_objects's of the board board_i(ash_turn[i]) under the batch's topology: the recipe that
 * reproduces it is golhip_batch_search_census's.  A soup without a repeat within max_turns has ash_turn
 * -1 and nobjects 0.  Errors: golhip_batch_search's checks, then golhip_batch_objects's checks of
 * max_objects and reach, in their words, all before any device work.  Side effects and independence
 * are golhip_batch_search_census's: no output for soup i depends on nsoups, the soup's position, the
 * chunking, GOLHIP_STAGE_BYTES or max_objects. */
int golhip_batch_search_objects(golhip_batch_t b, int64_t nsoups, const uint64_t *seeds /* nsoups, or NULL */,
                                uint64_t seed0, uint32_t density_q32, int64_t max_turns,
                                const uint32_t *birth /* nsoups, or NULL */, const uint32_t *survive,
                                int max_objects, int reach,
                                golhip_soup_t *out /* nsoups */, int64_t *cycle_start /* nsoups */,
                                int64_t *ash_turn /* nsoups */, int32_t *nobjects /* nsoups */,
                                golhip_object_t *objects /* nsoups * max_objects, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GOLHIP_H */
