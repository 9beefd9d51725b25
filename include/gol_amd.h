/*
 * gol_amd.h — C ABI of the MI355X-native Game of Life engine (libgolamd.so).
 *
 * Drop-in boundary for the reference's per-turn board update
 * (joyce-leesw/Conway-s-GOL-Distributed).  The reference crosses this boundary
 * with Go net/rpc calls whose payload is a gob-encoded [][]uint8 board; here it
 * is a plain C ABI (opaque handles, pointers + sizes, int error codes, no
 * exceptions and no torch types), so a cgo / ctypes / JNI binding is a thin stub
 * (INTEGRATION.md shows the cgo one).
 *
 * Two layers:
 *
 *  1. Engine (gol_ctx): one MI355X, one board or one row strip of a board.
 *     Owns every device buffer (double-buffered bit-packed board, 64 cells per
 *     uint64 word, LSB = lowest x; optional non-binary "blocked" mask; popcount
 *     shards).  Replaces, per GPU:
 *       API.SubServerDistributor          SubServer/distributor.go:48-84
 *       calculateNextState                SubServer/distributor.go:119-208
 *       the Server turn loop + commit     Server/gol/distributor.go:104-134
 *       API.Alivecount / calculateAliveCells  Server/gol/distributor.go:69-75,173-183
 *       API.GetWorld                      Server/gol/distributor.go:62-67
 *       Local calculateAliveCells         Local/gol/distributor.go:229-239
 *
 *  2. Run driver (gol_run): the C++ host mirror of
 *       gol.Run(Params, events chan<- Event, keyPresses <-chan rune)
 *                                         Local/gol/gol.go:12-40
 *     with the distributor's event sequence (Local/gol/distributor.go:55-227),
 *     the 2 s AliveCellsCount ticker (:58,154-167), the s/p/q/k key handling
 *     (:107-152, Server/gol/distributor.go:136-164) and the PGM I/O goroutine
 *     (Local/gol/io.go:42-143).
 *
 * Threading: one thread drives an engine (gol_step, loads, halo calls).  The read-only
 * calls (gol_snapshot, gol_get_info, gol_read_board, gol_get_world, gol_read_packed,
 * gol_alive_cells, gol_flipped_cells, gol_turn_counts, gol_read_window, gol_window_density,
 * gol_board_layout) may come from other threads at any time: during a gol_step the stepping
 * thread serves them at its next launch boundary, on a turn-consistent board; while the
 * step is parked on GOL_CONTROL_PAUSE they run at once (the reference Server's mutex is
 * held only around the per-turn commit: Server/gol/distributor.go:62-75,131-134).  A run
 * driver owns its engines on its own thread; gol_run_* calls are thread-safe.
 *
 * Return codes: GOL_OK or a negative GOL_E* code; gol_step returns GOL_STOPPED (> 0) when
 * the control word stopped it, gol_last_launches a count.  Test failures with rc < 0.
 * GOL_EHIP also reports a corrupt board: a k_step_wg pipeline wait that gave up (a starved
 * workgroup) sets the engine's device error word, and every synchronising call fails until
 * the board is replaced (gol_load*, gol_fill_random).
 */
#ifndef GOL_AMD_H
#define GOL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ error codes */
#define GOL_OK          0
#define GOL_EINVAL     -1   /* bad argument (size, null pointer, W < 2, ...)        */
#define GOL_EHIP       -2   /* HIP runtime error (message in gol_last_error)         */
#define GOL_ENOMEM     -3   /* device or host allocation failed                      */
#define GOL_ESTATE     -4   /* call not valid now (e.g. halo exhausted in strip mode)*/
#define GOL_ENODEV     -5   /* no usable HIP device                                  */
#define GOL_EIO        -6   /* PGM file missing / malformed (reference: panic)       */
#define GOL_ECLOSED    -7   /* run driver: event channel closed                      */
#define GOL_ETIMEDOUT  -8   /* run driver: no event within the timeout               */
#define GOL_STOPPED     1   /* gol_step returned early on GOL_CONTROL_STOP (not an error:
                               the turns done so far are in gol_info.turn)            */

/* ----------------------------------------------------------------- engine */
typedef struct gol_ctx gol_ctx;

/* flags */
#define GOL_FLAG_COUNT_EVERY_TURN  0x1u  /* record the alive count of every turn (gol_turn_counts).
                                            The count is fused into the one-turn stencil and into
                                            k_step_tile: an engine whose multi-turn kernel is
                                            k_step_tile at a gol_tile_count_codes code keeps its
                                            temporal blocking, every other one runs one turn per
                                            launch -- among them every engine whose width is no
                                            multiple of 128 (k_step_tile has no counted form
                                            across the row seam) */
#define GOL_FLAG_FORCE_GENERIC     0x2u  /* use the generic stencil even when the fast one applies */
#define GOL_FLAG_NO_AUTOTUNE       0x4u  /* skip the create-time (turns per launch, band) timing
                                            sweep on large boards (results never depend on it) */
#define GOL_FLAG_RESIDENT          0x8u  /* a request: run a torus board narrower than 256 cells
                                            resident in the registers of one workgroup, up to 256
                                            turns per launch (k_step_resident).  Eligible: halo ==
                                            0, width <= 255, height <= 256 x floor(16 / words per
                                            row) (4096, 2048, 1280, 1024 rows at 1 .. 4 words), no
                                            GOL_FLAG_FORCE_GENERIC, turns_per_launch != 1.  Every
                                            other engine runs as without the flag;
                                            gol_info.turns_per_launch tells which it got (the
                                            resident depth, or 1).  Results never depend on it. */

typedef struct gol_config {
    int32_t  width;       /* Params.ImageWidth  (>= 2)                                   */
    int32_t  height;      /* Params.ImageHeight of the WHOLE board (>= 1)                */
    int32_t  device;      /* HIP device ordinal; -1 = current device                     */
    int32_t  row_offset;  /* first global row owned by this engine                        */
    int32_t  rows;        /* rows owned; rows == height and halo == 0 => torus engine      */
    int32_t  halo;        /* strip mode: halo depth K in rows (1 <= K <= rows)            */
    uint32_t flags;       /* GOL_FLAG_*                                                   */
    int32_t  band_rows;   /* rows per wavefront band in the stencil; 0 = auto             */
    int32_t  turns_per_launch; /* temporal blocking: turns fused per stencil pass (1 = off;
                                  0 = default); results are identical for every value.
                                  Widths of at least 256 cells block: multiples of 128 on
                                  every multi-turn kernel, the others on k_step_tile alone
                                  (gol_tile_seam_codes where width % 64 != 0); narrower
                                  boards run one turn per launch unless GOL_FLAG_RESIDENT
                                  (then 0 = 256, and 2 .. 256 are taken).  A board buffer of 2 GiB
                                  or more blocks on k_step_tile alone (gol_tile_big_codes),
                                  and only with width % 64 == 0 and no per-turn counts
                                  (gol_info.blocking_limited)                            */
} gol_config;

typedef struct gol_info {
    int32_t  width, height, row_offset, rows, halo;
    int32_t  words_per_row;     /* ceil(width / 64)                                  */
    int32_t  pitch_words;       /* row stride of the device board in uint64 words    */
    int32_t  buffer_rows;       /* rows + 2 * halo                                   */
    int32_t  fast_path;         /* 1 = the LDS-free DPP stencil (width % 128 == 0, >= 256) */
    int32_t  band_rows;         /* effective band height                              */
    int32_t  halo_valid;        /* strip mode: turns left before the next exchange    */
    int32_t  turns_per_launch;  /* effective temporal-blocking depth (1: widths below 256
                                   unless GOL_FLAG_RESIDENT took effect,
                                   forced-generic engines, count engines of a width that
                                   is no multiple of 128, blocking_limited)             */
    int32_t  device;
    int64_t  turn;              /* completed turns since load                          */
    int64_t  nonbinary_cells;   /* cells that were neither 0 nor 255 at load           */
    int64_t  launches;          /* stencil kernel launches since load                  */
    int32_t  blocking_limited;  /* 1 = temporal blocking is off because a board buffer is
                                   >= 2 GiB and the engine is one that k_step_tile's big form
                                   (buffer resources rebased per tile: gol_tile_big_codes)
                                   does not run -- a count engine, a width that is no
                                   multiple of 64 or below 256, a forced-generic engine:
                                   every launch runs one turn.  Every other engine of that
                                   size blocks, on tiles whose rows (tile height + 2 x
                                   depth) span less than 2 GiB                          */
    int32_t  shape_source;      /* where the multi-turn launch shape came from: 0 = defaults
                                   or the caller (gol_config / GOL_* experiments), 1 = the
                                   create-time timing search, 2 = the pinned table of
                                   MI355X shapes for the BASELINE board sizes            */
} gol_info;

/* Whole-board (torus) engine on the current device. */
int  gol_create(int32_t width, int32_t height, uint32_t flags, gol_ctx **out);
/* Whole-board or row-strip engine (see gol_config). */
int  gol_create_ex(const gol_config *cfg, gol_ctx **out);
void gol_destroy(gol_ctx *ctx);
const char *gol_last_error(const gol_ctx *ctx);   /* per engine; "" if none            */
const char *gol_strerror(int code);
/* Build stamp: 16 hex digits of the sha256 of the library's sources (csrc/Makefile SRCS), so
 * a test can tell a library built from other sources than the tree it ships with. */
const char *gol_source_id(void);
int  gol_get_info(gol_ctx *ctx, gol_info *info);

/* Stream: the engine creates its own HIP stream; gol_set_stream makes it enqueue
 * on the caller's stream instead (e.g. torch.cuda.current_stream().cuda_stream).
 * NULL restores the engine's own stream. */
int   gol_set_stream(gol_ctx *ctx, void *hip_stream);
void *gol_get_stream(gol_ctx *ctx);
int   gol_sync(gol_ctx *ctx);

/* Load a board from host bytes (0 = dead, 255 = alive, anything else: the
 * reference's non-binary semantics).  Torus engine: height x width bytes.
 * Strip engine: (rows + 2*halo) x width bytes = global rows
 * row_offset-halo .. row_offset+rows+halo-1 (mod height).  Resets turn to 0. */
int gol_load(gol_ctx *ctx, const uint8_t *bytes);
/* Synthetic board: word (y, j) = splitmix64((seed << 40) + y*words_per_row + j),
 * y the GLOBAL row (oracle/bitref.c uses the same definition).  Resets turn. */
int gol_fill_random(gol_ctx *ctx, uint64_t seed);
/* Load / read packed words for the buffer rows (strip: incl. halos), row stride
 * words_per_row, for checkers that work on packed boards.  Packed words crossing
 * the ABI (here, gol_read_packed and the halo rows of gol_export_halo /
 * gol_import_halo) are always in the standard layout (cell x = bit x % 64 of word
 * x / 64), whatever internal layout the temporal-blocking kernel runs on.
 * Padding rule: when width % 64 != 0, the bits past `width` in the last word of every row
 * must be 0 (the stencil reads them as neighbours, and the counts and the alive list would
 * include them).  gol_load_packed checks every buffer row on the host before it copies:
 * a set padding bit returns GOL_EINVAL, gol_last_error names the row, and the engine's
 * board and turn stay as they were.  gol_read_packed and gol_export_halo always write
 * zero padding. */
int gol_load_packed(gol_ctx *ctx, const uint64_t *words);

/* Advance `turns` turns.  Torus engine: any turns >= 0.  Strip engine:
 * turns <= halo_valid (then exchange halos; see gol_export_halo).  Returns GOL_OK, or
 * GOL_STOPPED when the control word (below) said stop between two launches. */
int gol_step(gol_ctx *ctx, int64_t turns);

/* Control word, the engine-level mirror of the reference's CFput flag handshake
 * (Server/gol/distributor.go:54-60,136-164): any thread may set it at any time, without
 * the engine lock.  gol_step reads it before every kernel launch (a launch fuses up to
 * turns_per_launch turns): RUN continues, PAUSE parks gol_step at that launch boundary
 * with the board complete until the word changes, STOP makes gol_step return GOL_STOPPED.
 * Once an engine has seen gol_set_control, gol_step keeps at most 2 launches queued so
 * the word takes effect within 2 launches.  The word stays set until changed. */
#define GOL_CONTROL_RUN    0
#define GOL_CONTROL_PAUSE  1
#define GOL_CONTROL_STOP   2
int gol_set_control(gol_ctx *ctx, int32_t word);

/* The launches the last gol_step / gol_step_overlap call ran (planner introspection for
 * benchmarks and tests; no reference counterpart): up to `cap` entries of turns fused, kernel
 * (the engine's temporal-blocking kernel id; turns == 1: the one-turn stencil, kernel 0) and
 * band rows.  Returns the number of launches (may exceed cap; entries past 4096 are not
 * recorded), or a negative GOL_E* code. */
int gol_last_launches(gol_ctx *ctx, int32_t *turns, int32_t *kernel, int32_t *band, int32_t cap);
/* The same launches' k_step_tile shapes (kernel 15, and 16 = the same tiles resident across
 * blocks of turns): tile width in lanes, the segment code (SEG + 100 * turn order + 1000 *
 * (words per lane - 1)), the waves per workgroup and the turns per block (kernel 15: the
 * launch's turns); 0 for the other kernels.  Returns the launch count like
 * gol_last_launches. */
int gol_last_launch_tiles(gol_ctx *ctx, int32_t *tile_w, int32_t *tile_seg, int32_t *waves,
                          int32_t *block_turns, int32_t cap);
/* The chunk kernels the last gol_step ran: a long torus step cuts consecutive k_step_tile
 * launches into row chunks on two streams so that one chunk's tail, stores and loads run under
 * another's turns (GOL_STEP_CHUNKS in the environment, read per gol_step: 1 = off, n >= 2 = n
 * chunks per launch, unset or 0 = automatic).  0: every launch ran as one kernel.
 * gol_last_launches still reports one entry per launch.  Or a negative GOL_E* code. */
int gol_last_step_chunks(gol_ctx *ctx);
/* The chunk plan of two consecutive launches over `rows` buffer rows of a torus: the previous
 * one of k_prev turns on tiles of tile_h_prev rows asked for chunks_prev chunks, the next one
 * likewise.  counts[0..1]: the chunks each gets (cut on multiples of its tile height, every
 * chunk at least max(k_prev, k_next) rows tall: fewer than asked when they would not be);
 * prev_bounds / next_bounds: counts[i] + 1 row bounds; deps[q * cap + p] = 1 when chunk q of
 * the next launch must follow chunk p of the previous one.  cap >= both requests: the arrays
 * hold cap + 1 bounds and cap x cap bytes.  Needs no device. */
int gol_step_chunk_plan(int32_t rows, int32_t k_prev, int32_t tile_h_prev, int32_t chunks_prev,
                        int32_t k_next, int32_t tile_h_next, int32_t chunks_next, int32_t *counts,
                        int32_t *prev_bounds, int32_t *next_bounds, uint8_t *deps, int32_t cap);
/* The k_step_tile segment codes this library runs (planner introspection for the parity
 * tests: every code the shape search can pick has an oracle test).  Writes min(n, cap) codes,
 * returns n.  Needs no device. */
int gol_tile_codes(int32_t *codes, int32_t cap);
/* The workgroups of one k_step_tile launch of `turns` turns over `rows` rows of nw words, on
 * tiles of tile_h rows x tile_w lanes with segment code seg: grid[0] x grid[1] full-width
 * tiles (columns x rows) and, when the ragged last tile column is repacked at its own width,
 * grid[2] narrow tiles of grid[3] lanes x grid[4] rows in its place (else grid[2..4] = 0 and
 * grid[0] counts every column).  GOL_TILE_REPACK=0 in the environment turns the repack off.
 * Needs no device.  GOL_EINVAL for a shape the library does not run. */
int gol_tile_grid(int32_t nw, int32_t rows, int32_t turns, int32_t tile_h, int32_t tile_w,
                  int32_t seg, int32_t *grid);
/* The subset with a counted form (k_step_tile with the per-turn alive counts fused): the codes
 * a GOL_FLAG_COUNT_EVERY_TURN engine runs multi-turn launches on; same convention. */
int gol_tile_count_codes(int32_t *codes, int32_t cap);
/* The subset with a form for boards whose width is no multiple of 64 (k_step_tile across the
 * row seam: the torus wraps in x inside the row's last word): the codes such an engine runs
 * multi-turn launches on; same convention. */
int gol_tile_seam_codes(int32_t *codes, int32_t cap);
/* The subset with a form for board buffers of 2 GiB and more (k_step_tile_big: every tile
 * addresses its own window of rows through 64-bit bases, so no byte offset depends on the
 * buffer's size): the codes such an engine runs multi-turn launches on, width % 64 == 0 and no
 * per-turn counts; same convention.  GOL_TILE_BIG=1 in the environment at create forces the form
 * on a buffer of any size (tests, A/B runs); the create then fails with GOL_EINVAL for an
 * engine or shape the form does not run. */
int gol_tile_big_codes(int32_t *codes, int32_t cap);
/* The rows such a tile touches: a tile at buffer row y0 (0 <= y0 < modrows) of tile_h rows, run
 * `turns` turns deep on a buffer of modrows rows of pitch_words words, reads rows
 * (y0 - turns + j) mod modrows, j = 0 .. tile_h + 2 turns - 1: *rows_a rows from row *row0 on,
 * then *rows_b rows from row 0 on (0 unless the window wraps past the last row).
 * *base_a_bytes = *row0 x pitch_words x 8, the first part's byte distance from the buffer's
 * start (64-bit).  Needs no device.  GOL_EINVAL for a window of 2 GiB or more, for
 * modrows < tile_h + 2 turns (a window that would wrap twice) and for arguments out of range. */
int gol_tile_window(int64_t modrows, int64_t pitch_words, int64_t y0, int32_t turns,
                    int32_t tile_h, int64_t *row0, int64_t *rows_a, int64_t *rows_b,
                    uint64_t *base_a_bytes);
/* The word a k_step_tile lane holds at virtual lane column v of a row of `width` cells: cells
 * 64 v .. 64 v + 63 (mod width), bit b = cell 64 v + b.  row: the row's ceil(width / 64) words
 * (padding bits zero) in `layout` (0 standard, 1 interleaved: even cells in the low dword, odd
 * cells in the high one); *out is in the same layout.  v in [-1, words per row]: the columns a
 * tile no wider than the row loads.  This is the host build of the kernel's own stitch.
 * GOL_EINVAL for a v outside that range, width < 256, an unknown layout or null pointers.
 * Needs no device. */
int gol_seam_word(const uint64_t *row, int32_t width, int32_t v, int32_t layout, uint64_t *out);
/* How k_step_resident (GOL_FLAG_RESIDENT) partitions a torus board of width x height cells over
 * the lanes of its one workgroup: *lanes active lanes (1 .. 256) of *rows_per_lane consecutive
 * rows each -- the last lane owns what is left, at least one row -- in *waves wavefronts
 * (ceil(lanes / 64)); a lane holds rows_per_lane x ceil(width / 64) <= 16 words.  Needs no
 * device.  GOL_EINVAL for a board that is not eligible by its shape (width < 2 or > 255, height
 * < 1 or above 256 x floor(16 / words per row)) and for null pointers. */
int gol_resident_plan(int32_t width, int32_t height, int32_t *lanes, int32_t *rows_per_lane,
                      int32_t *waves);
/* The host build of k_step_resident: `turns` turns (>= 0) of the torus board `in` (height rows of
 * ceil(width / 64) words, standard layout, padding bits zero) into `out`, by the kernel's own
 * functions -- the partition above, the in-lane west / east words, the row sums, the rule, the
 * tail mask -- run lane by lane, with arrays indexed like the kernel's LDS exchange area (by lane
 * modulo the active lanes, double-buffered by turn parity).  counts: NULL, or `turns` entries,
 * the alive cells after each turn.  Needs no device.  GOL_EINVAL as gol_resident_plan. */
int gol_resident_host_run(const uint64_t *in, int32_t width, int32_t height, int32_t turns,
                          uint64_t *out, int64_t *counts);
/* The subset of those the persistent tile kernel (K1p: small torus boards, tiles resident
 * across blocks of turns) runs; same convention. */
int gol_tile_persist_codes(int32_t *codes, int32_t cap);
/* The subset the streamed tile kernel (K1q: large torus boards, blocks of turns over
 * (block, tile) items taken in order by resident workgroups) runs; same convention.  Empty
 * in the product library (K1q is a tools-build experiment). */
int gol_tile_stream_codes(int32_t *codes, int32_t cap);
/* Lock-free progress read for a controlling thread: *turn = turns enqueued so far (the
 * board reaches it at the next gol_sync), *parked = 1 while gol_step is parked on PAUSE
 * (the board is then complete at *turn).  Either pointer may be NULL. */
int gol_get_progress(gol_ctx *ctx, int64_t *turn, int32_t *parked);

/* Halo exchange overlapped with compute (strip engines; the zero-copy path of
 * gol_halo_buffers).  gol_stream_wait makes `hip_stream` (the transport's stream) wait for
 * the work queued on the engine so far -- the send rows are final.  The caller then
 * enqueues its sends and receives on that stream and calls gol_step_overlap, which marks
 * the halos fresh and advances `turns` (<= halo) turns: the first launch's interior rows
 * (those whose dependency cone stays inside the owned rows) start on the engine stream at
 * once, the rows next to the halos run on a second engine stream after the work queued on
 * `recv_stream`, and the engine stream joins it before the next launch.  Replaces the
 * reference's blocking fan-out / gather of every strip every turn
 * (Server/gol/distributor.go:118-129). */
int gol_stream_wait(gol_ctx *ctx, void *hip_stream);
int gol_step_overlap(gol_ctx *ctx, int64_t turns, void *recv_stream);

/* Consistent (turn, alive) pair of the current board (owned rows only). */
int gol_snapshot(gol_ctx *ctx, int64_t *turn, int64_t *alive);
/* Per-turn alive counts recorded by GOL_FLAG_COUNT_EVERY_TURN for turns
 * first_turn .. first_turn+n-1 (must be among the last 4096 turns: turn-4095 .. turn, else
 * GOL_EINVAL).  Every turn it accepts has its true count, also when called from another thread
 * during a gol_step or after one that GOL_CONTROL_STOP ended early. */
int gol_turn_counts(gol_ctx *ctx, int64_t first_turn, int64_t n, int64_t *out);

/* Owned rows as bytes (rows x width, 0/255; at turn 0 the loaded bytes as-is,
 * matching the reference's Turns = 0 output). */
int gol_read_board(gol_ctx *ctx, uint8_t *out);
/* GetWorld (Server/gol/distributor.go:62-67, the reply ItemW{SWorld, TurnCur}): the owned
 * rows as bytes, as gol_read_board, and the turn that board is at -- one consistent pair,
 * callable from another thread while gol_step runs (served at a launch boundary) or is
 * parked.  The 's' key of a controller that runs the whole game in one gol_step uses it. */
int gol_get_world(gol_ctx *ctx, uint8_t *out, int64_t *turn);
/* Owned rows as packed words (rows x words_per_row). */
int gol_read_packed(gol_ctx *ctx, uint64_t *out);
/* Row-major alive-cell list {x, y} (y = global row) of the owned rows, as
 * int64 pairs; writes min(n, cap) pairs and sets *n to the total. */
int gol_alive_cells(gol_ctx *ctx, int64_t *xy, int64_t cap, int64_t *n);
/* CellFlipped (Local/gol/event.go:47-57): the cells of the owned rows whose state differs
 * between the current board and the board one turn earlier, as row-major {x, y} int64 pairs
 * (y = global row); writes min(n, cap) pairs and sets *n to the total (cap == 0 or *n == 0:
 * xy is not touched).  Computed on the device from the two halves of the double buffer, so it
 * is valid only while the other half still holds the board exactly one turn back: after a
 * gol_step(ctx, 1) or gol_step_overlap(ctx, 1, ..) (a gol_step of 0 turns changes nothing),
 * until the next gol_load / gol_load_packed / gol_fill_random, a step of more than one turn, or
 * a gol_halo_buffers that converts the board to the interleaved layout; halo imports keep it
 * valid.  Otherwise GOL_ESTATE.  A flip is a change of the packed bit (bit set <=> byte ==
 * 255): a cell loaded with a byte that is neither 0 nor 255 has bit 0 before the first turn
 * and is dead after it, so it is not reported on that turn although its byte changed (the run
 * driver compares that one turn's bytes on the host). */
int gol_flipped_cells(gol_ctx *ctx, int64_t *xy, int64_t cap, int64_t *n);

/* ---- Windows: read, count and write a rectangle of the board at a cost proportional to the
 * rectangle (the whole-board calls above need width x height host bytes -- 16 GiB at 131072^2 --
 * and convert the whole buffer to the standard layout first; these work on the board in
 * whichever layout it is in and touch no row outside the window).  No reference counterpart: its
 * view is one pixel per cell (Local/sdl), its boards cross the RPC boundary whole.
 * A window is w x h cells whose top-left cell is (x, y) in GLOBAL board coordinates:
 * 0 <= x < width, 0 <= y < height, 1 <= w <= width, 1 <= h <= height.  Column x + i means
 * (x + i) mod width and row y + j means (y + j) mod height: a window may cross either wrap, and
 * never covers a cell twice.  Arguments out of range: GOL_EINVAL, the engine untouched.
 *
 * gol_read_window: h x w bytes (0 / 255, row stride w), exactly that window of what
 * gol_read_board returns (at turn 0 of a non-binary load: the loaded bytes as they are); *turn
 * (may be NULL) is the turn of that board.  A read-only call: from another thread during a
 * gol_step it is served at a launch boundary.  Strip engine: every window row must be an owned
 * row (row_offset <= y and y + h <= row_offset + rows), else GOL_EINVAL.  The board's layout
 * (gol_board_layout) stays as it is. */
int gol_read_window(gol_ctx *ctx, int32_t x, int32_t y, int32_t w, int32_t h, uint8_t *out,
                    int64_t *turn);
/* The window as alive counts per block x block cells, 1 <= block <= 4096 (a thumbnail of a
 * board too large to show): ceil(h / block) x ceil(w / block) counts, entry (J, I) = the alive
 * cells (packed bit set, as gol_snapshot counts) in window rows [J block, min(h, (J + 1) block))
 * x columns [I block, min(w, (I + 1) block)).  Threading and strip rule as gol_read_window. */
int gol_window_density(gol_ctx *ctx, int32_t x, int32_t y, int32_t w, int32_t h, int32_t block,
                       uint32_t *out, int64_t *turn);
/* Set the window's cells from h x w bytes: 255 = alive, any other value = dead (no non-binary
 * semantics; GOL_ESTATE while the engine holds the turn-0 board of a non-binary gol_load).  A
 * stepping-thread call, like the loads.  The turn, the launch count and the recorded per-turn
 * counts stay; the flip list becomes invalid (gol_flipped_cells: GOL_ESTATE until the next
 * one-turn step); padding bits stay 0.
 * Strip engine: every BUFFER row, owned or halo, whose global row (row_offset - halo + b) mod
 * height lies in the window is written -- both copies when the buffer holds a global row twice,
 * none (GOL_OK) when it holds none of the window's.  So a caller that applies the same call to
 * every strip of a board at a window boundary (after an exchange, before the next gol_step)
 * keeps the strips consistent: each strip's halo rows get what their owner's rows get. */
int gol_write_window(gol_ctx *ctx, int32_t x, int32_t y, int32_t w, int32_t h,
                     const uint8_t *bytes);
/* Every buffer row dead.  Resets what gol_load_packed resets: turn 0, standard layout, the
 * error word, halo_valid. */
int gol_clear(gol_ctx *ctx);
/* The layout the current board buffer is in now: 0 standard, 1 interleaved (what a multi-turn
 * gol_step leaves; the whole-board read-outs convert it back, the window calls do not). */
int gol_board_layout(gol_ctx *ctx);
/* The 64 cells at columns col .. col + 63 (mod width) of one row: bit b of *out = cell
 * (col + b) mod width, in standard order.  row: the row's ceil(width / 64) words in `layout`
 * (0 standard, 1 interleaved: even cells in the low dword, odd cells in the high one).  This is
 * the host build of the function the window kernels fetch their cells with.  With
 * r = width % 64 != 0 the 64 cells can span THREE words (the tail of word L - 1, the r cells of
 * the last word L, then word 0), and a row narrower than 64 cells wraps more than once.
 * GOL_EINVAL for null pointers, width < 2, col outside [0, width) or an unknown layout.  Needs no
 * device. */
int gol_window_word(const uint64_t *row, int32_t width, int32_t col, int32_t layout,
                    uint64_t *out);

/* Strip mode halo exchange.  export: copy the first and the last `halo` owned
 * rows (packed, halo x words_per_row uint64 each) to device buffers `top` and
 * `bottom` on `hip_stream` (NULL = engine stream).  import: copy the neighbour
 * rows into this engine's halos (top = the rows above, from rank r-1's bottom;
 * bottom = the rows below, from rank r+1's top) and reset halo_valid to halo.  The imported
 * rows obey gol_load_packed's padding rule (bits past `width` are 0); they are device memory,
 * so the engine cannot check them: rows written by gol_export_halo always comply. */
int gol_export_halo(gol_ctx *ctx, void *top, void *bottom, void *hip_stream);
int gol_import_halo(gol_ctx *ctx, const void *top, const void *bottom, void *hip_stream);
/* In-process exchange between two strip engines (any devices, peer copies):
 * dst's top halo <- src's last `halo` owned rows (src is dst's upper neighbour). */
int gol_copy_halo_from_upper(gol_ctx *dst, gol_ctx *src);
/* dst's bottom halo <- src's first `halo` owned rows (src is dst's lower neighbour). */
int gol_copy_halo_from_lower(gol_ctx *dst, gol_ctx *src);
/* Mark the halos fresh after all copies into this engine are enqueued. */
int gol_halo_done(gol_ctx *ctx);
/* Zero-copy exchange (the RCCL path: the transport reads and writes the board
 * itself).  Device pointers into the current board buffer: send_top / send_bottom =
 * the first / last `halo` owned rows, recv_top / recv_bottom = the top / bottom halo
 * rows, each halo x words_per_row uint64 with row stride words_per_row.  The rows
 * are in the engine's stepping layout (converted to it here if needed), returned in
 * *layout (0 standard, 1 interleaved): both ends of an exchange must report the
 * same layout -- engines created with the same width, halo and flags do.  The
 * pointers are valid until the next gol_step / gol_load*.  Order the transport after
 * the engine's stream, and the next gol_step after the receives, then call
 * gol_halo_done.  Replaces the per-turn strip+halo RPC copy
 * (reference Server/gol/distributor.go:185-224). */
int gol_halo_buffers(gol_ctx *ctx, void **send_top, void **send_bottom, void **recv_top,
                     void **recv_bottom, int32_t *layout);

/* ------------------------------------------------------------------ Batch
 * Many small boards in one launch (k_step_resident_batch).  A gol_batch owns `boards` torus
 * boards of one shape, width x height cells each, in one device buffer: board i's rows follow
 * board i - 1's, height x ceil(width / 64) words per board in the standard layout.  A step runs
 * ceil(turns / 256) launches of near-equal depth, each with one workgroup per board that keeps
 * its board in registers for the launch's turns (the partition of gol_resident_plan) and writes
 * it back in place: the batch has one buffer, no double buffer.  No reference counterpart (its
 * Server runs one board).
 *
 * Eligible shapes are gol_resident_plan's and nothing else -- width 2 .. 255, height at most
 * 4096 / 2048 / 1280 / 1024 rows at 1 .. 4 words per row; there is no fallback kernel -- with
 * boards >= 1 and boards x height <= INT32_MAX.  flags: 0 or GOL_FLAG_COUNT_EVERY_TURN (any
 * other bit: GOL_EINVAL).  device: -1 = the current device.  Arguments are checked before the
 * device is looked for: GOL_EINVAL, then GOL_ENODEV, then GOL_ENOMEM.  A new batch holds dead
 * boards at turn 0.
 *
 * Threading: one thread drives a batch.  There are no cross-thread services and no control
 * word.  Every call on a NULL handle returns GOL_EINVAL; gol_batch_last_error(NULL) is "". */
typedef struct gol_batch gol_batch;
int  gol_batch_create(int32_t width, int32_t height, int32_t boards, int32_t device,
                      uint32_t flags, gol_batch **out);
void gol_batch_destroy(gol_batch *b);
const char *gol_batch_last_error(const gol_batch *b);
/* The shape, the partition every board runs on (gol_resident_plan) and the turn.  Any
 * out-pointer may be NULL. */
int  gol_batch_get_info(gol_batch *b, int32_t *width, int32_t *height, int32_t *boards,
                        int32_t *words_per_row, int32_t *lanes, int32_t *rows_per_lane,
                        int32_t *waves, int64_t *turn);
/* How many of the batch's workgroups one launch keeps resident at once: *blocks_per_cu (the
 * occupancy the HIP runtime reports for this batch's kernel) on each of *cus compute units.  A
 * batch of more boards runs in rounds; results never depend on it (introspection for tests and
 * tools/batch_speed.py). */
int  gol_batch_occupancy(gol_batch *b, int32_t *blocks_per_cu, int32_t *cus);
/* The batch's own HIP stream, on which all its work is queued (for a caller that records events
 * around a step or orders other work after it); NULL for a NULL handle. */
void *gol_batch_get_stream(gol_batch *b);
int  gol_batch_sync(gol_batch *b);
/* Loads work on boards first .. first + n - 1 (n >= 1; a range outside the batch: GOL_EINVAL,
 * nothing changed) and leave the other boards as they are.  A load of the whole batch sets the
 * turn to 0; a partial load keeps it, so a caller can re-seed extinct boards mid-run.  While
 * counts are recorded, the count ring still holds what the board's previous occupant had at the
 * recorded turns: the entries of a partially loaded board before its load are the caller's
 * concern.
 * gol_batch_load_packed: n x height x words_per_row words.  gol_load_packed's padding rule
 * holds: a set bit past `width` in a row's last word returns GOL_EINVAL, gol_batch_last_error
 * names the board and the row, and nothing is copied.
 * gol_batch_load: n x height x width bytes, 255 = alive, anything else = dead (no non-binary
 * semantics, as gol_write_window).
 * gol_batch_fill_random: board i, row y = row i x height + y of what gol_fill_random(seed) gives
 * a board of width x (boards x height) cells; sets the turn to 0. */
int  gol_batch_load_packed(gol_batch *b, int32_t first, int32_t n, const uint64_t *words);
int  gol_batch_load(gol_batch *b, int32_t first, int32_t n, const uint8_t *bytes);
int  gol_batch_fill_random(gol_batch *b, uint64_t seed);
/* Advance every board `turns` turns (>= 0).  Asynchronous: the read-outs and gol_batch_sync
 * wait for it. */
int  gol_batch_step(gol_batch *b, int64_t turns);
/* Boards first .. first + n - 1 as n x height x words_per_row packed words (zero padding), as
 * n x height x width bytes (0 / 255), and as one alive count per board. */
int  gol_batch_read_packed(gol_batch *b, int32_t first, int32_t n, uint64_t *out);
int  gol_batch_read(gol_batch *b, int32_t first, int32_t n, uint8_t *out);
int  gol_batch_alive(gol_batch *b, int32_t first, int32_t n, int64_t *out);
/* Per-turn alive counts of a GOL_FLAG_COUNT_EVERY_TURN batch (else GOL_ESTATE): n x boards
 * entries, turn the major index, the counts after turns first_turn .. first_turn + n - 1.  Those
 * turns must be among the last 256 stepped turns (turn - 255 .. turn, and at least 1) and stepped
 * since the last whole-batch load, else GOL_EINVAL. */
int  gol_batch_turn_counts(gol_batch *b, int64_t first_turn, int64_t n, int64_t *out);

/* ------------------------------------------------------------------ Settle
 * Find the period of every board of a batch on the device, and skip the turns of a board known to
 * repeat (k_settle_resident_batch).  A batch can WATCH its boards.  While board i is watched from
 * turn start_i, the batch keeps a snapshot of it, taken at turns s_k = start_i + 2^k - 1, k = 0,
 * 1, 2, ... (Brent's schedule).  After every watched turn t the board is compared with its
 * current snapshot, every word of every row; at t == s_k + 2^k the compare comes first, and a
 * board that does not match becomes snapshot k + 1.  The first match gives period = t - s_k and
 * settled_turn = t.  That period is the minimal period of the cycle the board has entered: with
 * mu the first turn of the cycle, settled_turn = s_k + period for the least k with s_k >= mu and
 * 2^k >= period.  After its match a board is watched no more, and every later advance of d turns
 * runs d mod period turns on it (the rest of the launch the match was found in included).  A dead
 * board has period 1.  Neither the entries nor the boards depend on how a step is cut into
 * launches or on how many boards are resident at once.
 *
 * All boards of a batch stay at the batch's one turn: after gol_settle_step(b, n) every read-out
 * (gol_batch_read*, gol_batch_alive) equals what gol_batch_step(b, n) gives.
 *
 * gol_settle_step: advance every board `turns` turns (>= 0) like gol_batch_step, asynchronous
 * like it, watching as above.  The first call after a reset (below) starts the watch of every
 * board at the batch's turn then, with snapshot 0 = the board as it is; the watch's device
 * buffers (a snapshot and 32 bytes per board) are allocated at the first call.  A step runs
 * launches of at most 256 turns; GOL_SETTLE_DEPTH=D in the environment, read at every call,
 * makes that 1 .. 256 (tests put launch boundaries at every phase of the schedule with it).
 * turns < 0 or a NULL handle: GOL_EINVAL.  A batch created with GOL_FLAG_COUNT_EVERY_TURN:
 * GOL_ESTATE, and nothing runs (the per-turn count of a skipped turn is not recorded).
 *
 * gol_settle_read: one entry per board of first .. first + n - 1 (gol_batch_alive's range rule):
 * period 0 and settled_turn -1 while unknown.  Either out-pointer may be NULL.  GOL_ESTATE if no
 * watch is on.
 *
 * Resets: gol_batch_step, gol_batch_fill_random and a load of the whole batch end the watch of
 * all boards and forget their periods (the three calls themselves behave as without a watch); the
 * next gol_settle_step starts anew.  A partial load made while a watch is on restarts the watch
 * of the loaded boards at the batch's current turn; the other boards keep theirs. */
int  gol_settle_step(gol_batch *b, int64_t turns);
int  gol_settle_read(gol_batch *b, int32_t first, int32_t n, int64_t *settled_turn,
                     int64_t *period);
/* The host build of k_settle_resident_batch for one board: the kernel's own functions run lane
 * by lane on arrays indexed like its LDS areas, the waves' compare words, the reload of the state
 * at every launch and the skip of settled turns included (as gol_resident_host_run is for
 * k_step_resident).  `turns` turns from turn 0 in launches of at most `depth` turns (1 .. 256),
 * the watch starting at turn 0.  in / out: height x ceil(width / 64) words.  settled_turn and
 * period (either may be NULL) as gol_settle_read.  GOL_EINVAL for NULL in / out, turns < 0, a
 * depth outside 1 .. 256 and a shape gol_resident_plan refuses.  Needs no device. */
int  gol_settle_host_run(const uint64_t *in, int32_t width, int32_t height, int64_t turns,
                         int32_t depth, uint64_t *out, int64_t *settled_turn, int64_t *period);

/* -------------------------------------------------------------- run driver */
typedef struct gol_params {          /* Local/gol/gol.go:4-9 */
    int64_t turns;
    int32_t threads;                 /* kept for API parity; the GPU result is independent of it */
    int32_t image_width;
    int32_t image_height;
} gol_params;

typedef enum gol_event_type {        /* Local/gol/event.go:9-68 */
    GOL_EV_ALIVE_CELLS_COUNT    = 1,
    GOL_EV_IMAGE_OUTPUT_COMPLETE = 2,
    GOL_EV_STATE_CHANGE         = 3,
    GOL_EV_CELL_FLIPPED         = 4,
    GOL_EV_TURN_COMPLETE        = 5,
    GOL_EV_FINAL_TURN_COMPLETE  = 6
} gol_event_type;

typedef enum gol_state { GOL_PAUSED = 0, GOL_EXECUTING = 1, GOL_QUITTING = 2 } gol_state;

typedef struct gol_event {
    int32_t type;                    /* gol_event_type                                  */
    int32_t new_state;               /* StateChange.NewState                            */
    int64_t completed_turns;         /* every event's GetCompletedTurns()               */
    int64_t cells_count;             /* AliveCellsCount.CellsCount; FinalTurnComplete: len(Alive) */
    int64_t x, y;                    /* CellFlipped.Cell                                */
    char    filename[256];           /* ImageOutputComplete.Filename                    */
} gol_event;

typedef struct gol_run_options {
    const char *image_dir;           /* where {W}x{H}.pgm is read ("images")            */
    const char *out_dir;             /* where {W}x{H}x{T}.pgm is written ("out")        */
    int32_t ngpus;                   /* row strips = engines (the reference's len(SUB)); 0 = 1 */
    const int32_t *devices;          /* exactly ngpus device ordinals (the array is read at
                                        indices 0..ngpus-1); NULL = 0..ngpus-1 (mod count)  */
    int32_t halo;                    /* strip halo depth K; 0 = auto                    */
    int32_t ticker_ms;               /* AliveCellsCount period; 0 = 2000 (distributor.go:58) */
    int32_t event_capacity;          /* bounded event channel; 0 = 1 (unbuffered-like)  */
    int32_t emit_turn_complete;      /* 1 = TurnComplete{t} for every turn (event.go:55-60) */
    int32_t emit_cell_flipped;       /* 1 = CellFlipped for initial cells and each flip  */
    uint32_t engine_flags;           /* GOL_FLAG_* for the engines                      */
    int32_t resume;                  /* 1 = CONT=yes (Local/gol/distributor.go:171-178): continue
                                        from the board and turn the previous run in this
                                        process ended with (the reference Server's retained
                                        world/turn), running Turns - turn more turns; -1 =
                                        read the CONT environment variable                 */
} gol_run_options;

typedef struct gol_run gol_run;

/* Start a run (non-blocking, like gol.Run).  opts may be NULL (defaults). */
int gol_run_start(const gol_params *p, const gol_run_options *opts, gol_run **out);
/* Receive the next event: GOL_OK, GOL_ECLOSED once the channel is closed and
 * drained, GOL_ETIMEDOUT after timeout_ms (< 0 = wait forever). */
int gol_run_next_event(gol_run *r, gol_event *ev, int32_t timeout_ms);
/* FinalTurnComplete.Alive of the most recently received FinalTurnComplete:
 * writes min(n, cap) {x, y} int64 pairs, returns n (or < 0 on error). */
int64_t gol_run_final_alive(gol_run *r, int64_t *xy, int64_t cap);
/* keyPresses <- rune ('s', 'p', 'q', 'k'). */
int gol_run_key(gol_run *r, int32_t rune);
/* Error text of a run that failed (the events channel is closed early).  NULL: why the calling
 * thread's last gol_run_start failed after validating its arguments (e.g. GOL_EHIP: two strip
 * devices that report peer access but refuse to enable it); "" after a successful start. */
const char *gol_run_error(gol_run *r);
/* Join the driver thread and free the run. */
void gol_run_destroy(gol_run *r);

#ifdef __cplusplus
}
#endif
#endif /* GOL_AMD_H */
