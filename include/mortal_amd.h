/* mortal_amd — C-ABI of the MI355X-native batched riichi arena (drop-in for the hot path of Mortal's `libriichi`).
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  Device pointers are raw HIP device addresses
 * (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (0 = default stream).
 * Every function returns 0 on success or a negative code; mj_last_error() describes the failure.
 * A call that returns an error leaves the pool as it was before the call: nothing of a half-done call stays behind, and the
 * same call may be tried again.  (What a stream reports at a synchronise is a failure of work already queued on the device: the
 * host side of the pool is as it was, the tables are not.)  One exception: mj_pool_enable_log frees the old log before it
 * allocates the new one (a log may take a gigabyte) and on failure leaves the log disabled.
 *
 * Each entry point names the reference interface it replaces (paths relative to libriichi/src):
 *
 *   mj_tables_upload      algo/shanten.rs:11-44 + algo/agari.rs:24-51   (lazy-static table loading)
 *   mj_pool_create/reset  arena/game.rs:230-266  BatchGame::run set-up: one Game per (seed, seat plan)
 *                         arena/one_vs_three.rs:140-191  seed list / agent index planning (done by the caller)
 *   mj_pool_configure     agent/mortal.rs:53-74  engine attributes read once per agent
 *   mj_step               arena/game.rs:286-304  one poll/commit cycle over every live game:
 *                           Game::commit (game.rs:180-218) + agent/mortal.rs:292-573 get_reaction (action decode)
 *                           Game::poll   (game.rs:59-178)  + BoardState::poll/step (board.rs:141-161,511-678)
 *                           agent/mortal.rs:200-250 set_scene (quick-eval, kan-select classification)
 *   mj_rows_count         agent/mortal.rs:118-123  batch size of the coming react_batch call
 *   mj_encode             agent/mortal.rs:252-287 -> state/obs_repr.rs:126-630  obs + mask for every row of the batch
 *   mj_random_policy      (no reference counterpart: BASELINE config 2's uniform-random legal policy)
 *   mj_greedy_policy      (no reference counterpart: tenpai-seeking benchmark / test policy)
 *   mj_results            arena/result.rs:19-30 GameResult.scores; arena/one_vs_three.rs:55-60 ranking input
 *   mj_counters           arena/game.rs:298-311 cycles/actions progress counters
 *   mj_pool_stat, mj_stat_logs   stat.rs:263-441 Stat::from_game, summed as stat.rs:443-498 Stat::from_dir sums the games of a run
 *   mj_replay_load_pool   arena/result.rs:32-51 dump_json_log -> dataset/gameplay.rs:66-124 load_gz_log_files (the log files between
 *                         self-play and the loader), without the files: the arena's device log is the loader's script
 *   mj_pool_grp, mj_grp_logs     dataset/grp.rs:90-164 Grp::load_events
 *   MJ_LOAD_AUGMENT, mj_augment_logs   dataset/gameplay.rs:126-128 (augmented) -> mjai/event.rs:187-217 Event::augment, tile.rs:154-167
 *   mj_pool_enable_harvest, mj_harvest_pending, mj_harvest_take, mj_harvest_info / _games / _read / _destroy
 *                         arena/game.rs:291-296 (a finished game's GameResult is handed over while the others play on) +
 *                         arena/result.rs:19-51 (what a GameResult keeps: seed, scores, log)
 *   mj_harvest_stat       stat.rs:263-441 + 443-498, as mj_pool_stat      mj_harvest_grp   dataset/grp.rs:90-164, as mj_pool_grp
 *   mj_replay_load_harvest   arena/result.rs:32-51 -> dataset/gameplay.rs:66-124, as mj_replay_load_pool
 *   mj_samples_create / _destroy / _append / _truncate / _info / _meta   mortal/dataloader.py:45-113 (the buffer populate_buffer fills
 *                         and shuffles) over dataset/gameplay.rs:239-443 entries, kept as records
 *   mj_samples_encode, mj_samples_encode_oracle   state/obs_repr.rs:126-630, dataset/invisible.rs: the obs of buffered entries, on demand
 */
#ifndef MORTAL_AMD_H
#define MORTAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct MjPool MjPool;

enum { MJ_DEAL_RAND08 = 0, MJ_DEAL_RAND09 = 1 };

const char* mj_last_error(void);
int mj_abi_version(void);

/* Upload the lookup tables (payload format: mortal_amd/tables.py, 'MJT1').  Once per process and device. */
int mj_tables_upload(const void* payload, size_t size);

/* n_tables concurrent tables; obs `version` 1..4 (consts.rs:20-28); max_rows = capacity of the row lists per agent
 * (0 -> 8 * n_tables, the theoretical maximum). */
MjPool* mj_pool_create(int n_tables, int version, int deal_algo, int max_rows);
void mj_pool_destroy(MjPool* pool);

/* Start n_tables games.  Host arrays of length n_tables: seed nonce/key (board.rs:99-107), global game id, and
 * agent_of_seat (bit s = agent index 0/1 of seat s).  n_games_total sizes the result arrays (>= max game id + 1). */
int mj_pool_reset(MjPool* pool, const uint64_t* nonces, const uint64_t* keys, const uint32_t* game_ids,
                  const uint8_t* agent_of_seat, int n_games_total);

/* Per-agent engine attributes (agent/mortal.rs:53-74): obs version (0 = keep), quick-eval, agari guard. */
int mj_pool_configure(MjPool* pool, int agent, int version, int enable_quick_eval,
                      int enable_rule_based_agari_guard);
/* Per-table mjai event log (arena/board.rs:189-197 add_log -> arena/result.rs:32-51 dump_json_log), off by default.
 * words_per_table u64 words are reserved per table (a hanchan needs <= ~250 words per kyoku); a table that overflows
 * ends with error MJ_ERR_LOG_OVERFLOW (7).  Word format: mortal_amd/csrc/mj_state.h LG_*; decoded by mortal_amd/mjai_log.py. */
int mj_pool_enable_log(MjPool* pool, uint32_t words_per_table);
int mj_log_lengths(MjPool* pool, uint32_t* len_out /* [n_tables] host */, void* stream);
int mj_log_read(MjPool* pool, int table0, int n, uint64_t* words_out /* [n][words_per_table] host */, void* stream);

/* Steady-state mode for throughput runs: finished tables restart with nonce += stride. 0 disables. */
int mj_pool_set_refill(MjPool* pool, uint64_t nonce_stride);
/* Steady-state throughput mode only (after mj_pool_reset + mj_pool_set_refill, before the first mj_step): instead of all tables
 * starting their hanchan on the same cycle, table t enters play at cycle hash(t) % cycles (it is parked as finished until then
 * and started by the refill path), so a pool is spread over every phase of a hanchan from the start — what a long-running
 * self-play server looks like.  No reference counterpart (BatchGame::run starts all games at once and never restarts one). */
int mj_pool_set_start_stagger(MjPool* pool, uint32_t cycles, void* stream);

/* One arena cycle.  actions_dev[a] = int32 device array with one action id (0..45) per row of agent a's previous
 * batch (NULL on the first cycle or when that agent had no rows).
 * An id whose mask bit was clear puts that table -- and no other -- in error MJ_ERR_ILLEGAL_ACTION (1): it leaves play in this
 * step with done flag 2 (mj_results), is counted by counters [1] (games) and [2] (errors) and reported by mj_pool_first_error.
 * That includes every id outside 0..45, and 45 (pass) on a row whose seat cannot pass (an own-turn row: mask[45] clear).  This
 * is stricter than the reference, whose decoder ends in `_ => Event::None` (agent/mortal.rs:571-572): there a masked policy never
 * produces such an id and what follows one is an accident (the board takes "nobody reacted" and draws again for a seat that
 * never discarded), here a garbage answer -- a NaN q row under the agari guard selects 45 -- must end in a code, not in a game
 * that silently diverges. */
int mj_step(MjPool* pool, const int32_t* actions_dev0, const int32_t* actions_dev1, void* stream);
/* Same, with the q-values of each batch (f32 device array [n_rows][46], agent/mortal.rs:126,150).  Needed when an agent
 * was configured with enable_rule_based_agari_guard: an agari (action 43) that PlayerState::rule_based_agari
 * (state/agent_helper.rs:251-368) rejects is replaced by the best other action, exactly as agent/mortal.rs:319-336. */
int mj_step_q(MjPool* pool, const int32_t* actions_dev0, const int32_t* actions_dev1, const float* q_dev0,
              const float* q_dev1, void* stream);

/* The same with EXPLICIT reactions for an agent: ev_devN = one packed mjai event word per row of agent N's batch (the
 * header word of the LG_* log format, 0 = {"type":"none"}), applied verbatim instead of an action id — the reference's
 * MjaiLogBatchAgent (agent/mjai_log.rs:12-150, py_agent.rs:24-37) answers with events.  The host validates them first
 * (state/action.rs:91-228). */
int mj_step_ev(MjPool* pool, const int32_t* actions_dev0, const int32_t* actions_dev1, const float* q_dev0,
               const float* q_dev1, const uint64_t* ev_dev0, const uint64_t* ev_dev1, void* stream);

/* ---- Log replay for the dataset loader (dataset/gameplay.rs:239-443 Gameplay::load_events_by_player).
 * One game log per table, as packed event words (LG_* format, the same words mj_log_read returns; host encoder:
 * mortal_amd/mjai_log.py encode_events).  script = all logs concatenated, off[n_logs + 1] = word offsets, tracked[t] bit s =
 * samples wanted for seat s of log t.  mj_replay_step applies events until some tracked seat has a sample, then
 * mj_rows_count / mj_encode(agent 0) / mj_encode_oracle deliver obs + masks exactly as in the arena, and mj_replay_meta the
 * per-row int32[8] = {label, log, seat, kyoku index, turn, shanten, is kan-select row, event index}.
 * counters()[1] = logs fully replayed.
 * For the invisible obs (GameplayLoader(oracle=True), dataset/invisible.rs) a start_kyoku word may carry the whole wall
 * (LG_SK_WALL_BIT) or ask for it to be rebuilt from the table's seed (LG_SK_DEAL_BIT, nonces/keys given; trust_seed);
 * in replay mode mj_encode_oracle lists every undrawn yama tile like Invisible::encode. */
int mj_replay_load(MjPool* pool, const uint64_t* script_host, const uint32_t* off_host, const uint8_t* tracked_host,
                   int n_logs, int always_include_kan_select, const uint64_t* nonces_host /* NULL ok */,
                   const uint64_t* keys_host /* NULL ok */);
/* The same load, from the device log of another pool (arena/result.rs:32-51 dump_json_log + dataset/gameplay.rs:66-124
 * load_gz_log_files without the files and the JSON between them): log t of `dst` = the log of src's table table0 + t, for all
 * dst->n_tables tables, copied on the device.  A table whose game has not finished without an error (done != 1) gets an empty
 * script and is counted as skipped; one whose log_len exceeds the log's capacity or whose event chain runs past its end or meets an
 * unknown event type is counted as malformed and gets an empty script too.  counts_out = {loaded, skipped, malformed}.
 * tracked_host: [dst n_tables] seat masks, NULL = all four seats.  flags: MJ_LOAD_* below, 0 and 1 mean what the former
 * `int deal_from_seed` meant; any other bit is an error that leaves dst as it was.  MJ_LOAD_DEAL_FROM_SEED: every start_kyoku asks for
 * the wall to be rebuilt from the seed (LG_SK_DEAL_BIT) and dst's table t takes the seed of src's table table0 + t.  MJ_LOAD_AUGMENT:
 * the copy swaps manzu and pinzu in every tile field of the script (GameplayLoader(augmented=True), dataset/gameplay.rs:126-128:
 * Event::augment of every event -- dora marker and haipai of start_kyoku, pai / consumed of tsumo, dahai, dora, chi, pon, the three
 * kans, ura markers of hora; kyoku number, winds, scores, deltas and tag words stay); with both flags every start_kyoku also carries
 * LG_SK_AUG_BIT: the wall is dealt from the seed as it was and compared with the script through the swap (the reference's mix of
 * swapped events and an unswapped Invisible).  src's log is never changed.  Needs mj_pool_enable_log on src;
 * an error if src is in refill mode (a restarted table's log has been rewound; mj_replay_load_harvest is the route there), if src == dst or if the range leaves src.  Ordered
 * behind the steps of src already launched; synchronous; src is never modified.  Afterwards dst is where mj_replay_load leaves it. */
#define MJ_LOAD_DEAL_FROM_SEED 1
#define MJ_LOAD_AUGMENT 2
int mj_replay_load_pool(MjPool* dst, MjPool* src, int table0, const uint8_t* tracked_host /* NULL ok */,
                        int always_include_kan_select, int flags /* MJ_LOAD_* */, int64_t counts_out[3], void* stream);
int mj_replay_step(MjPool* pool, void* stream);
int mj_replay_meta(MjPool* pool, int32_t* meta_dev, void* stream);

/* ---- Single-table access behind libriichi.state.PlayerState (state/player_state.rs:142-167, tests / debugging):
 * apply one event (LG_* words, "?" tiles = 37 allowed for hidden hands), make (table, seat) the only policy row so that
 * mj_rows_count + mj_encode return its obs/mask (state/obs_repr.rs:776-791 encode_obs), and a few queries:
 * what = 0 agari_points(args: is_ron, n_ura, ura[5]) -> ok, ron, tsumo_ko, tsumo_oya | 1 rule_based_agari |
 *        2 real_time_shanten | 3 doras_owned[4] | 4 add_dora_indicator(args[0]) | 5 set scores(args[0..3]) |
 *        6 set_scene (agent/mortal.rs:200-250) | 7 action id -> event word (agent/mortal.rs:338-573) |
 *        8 the step kernel's check of an explicit reaction word (args: word lo, hi; state/action.rs:91-228 plus the seat
 *          the call is made on) -> error code (0 = accepted), reaction type; the table is left untouched. */
int mj_table_apply_event(MjPool* pool, int table, const uint64_t* words_host, int n_words, void* stream);
int mj_table_mark_row(MjPool* pool, int table, int seat, int at_kan_select, void* stream);
int mj_table_query(MjPool* pool, int table, int seat, int what, const int32_t* args8_host, int32_t* out8_host, void* stream);

/* Number of policy rows per agent produced by the last mj_step.  Waits for the row counts of THAT step (recorded on the stream the
 * step was launched on; `stream` is only used before any step has run) -- it does NOT drain the stream: the snapshot kernel queued
 * behind the counts may still be running when the call returns.  mj_encode / mj_encode_oracle order themselves behind it: on the
 * step's stream by stream order, on any other stream by waiting for the snapshot's event.
 * Fails with "row capacity exceeded" when a batch has more rows than the pool's max_rows: n_rows_out is still filled in, the batch
 * stays invalid and mj_encode / mj_encode_oracle / mj_replay_meta refuse it until the next successful mj_rows_count. */
int mj_rows_count(MjPool* pool, int32_t n_rows_out[2], void* stream);
/* Device array of row descriptors of agent a: table | seat << 28 | is_kan_select << 31. */
const uint32_t* mj_rows_dev(MjPool* pool, int agent);

/* Encode agent a's rows: obs_dev [n_rows][C][34] f32, masks_dev [n_rows][46] u8 (bool). */
int mj_encode(MjPool* pool, int agent, float* obs_dev, uint8_t* masks_dev, void* stream);
/* Invisible ("oracle") observation of agent a's rows, for engines with is_oracle=True (arena/game.rs:100-101 ->
 * BoardState::encode_oracle_obs, arena/board.rs:679-782): out_dev [n_rows][mj_oracle_obs_rows(version)][34] f32. */
int mj_encode_oracle(MjPool* pool, int agent, float* out_dev, void* stream);
/* consts.rs:32-38 oracle_obs_shape(version).0: 211 for v1, 217 for v2..v4, -1 otherwise. */
int mj_oracle_obs_rows(int version);
/* Average duration (ms) of the encode kernel launches timed with HIP events since the last call, and their count. */
int mj_encode_timing(MjPool* pool, int enable, double* total_ms_out, int64_t* launches_out);
/* Same for the SP-table kernel (obs v4 rows 889..1011) launched by mj_encode; collected while encode timing is enabled. */
int mj_sp_timing(MjPool* pool, double* total_ms_out, int64_t* launches_out);
/* Cumulative phase timers of mj_k_sp since the pool was created (workgroup wall-clock ticks at 100 MHz, summed over all
 * workgroups): out[0] hash/pool overflows, [1] rows, [2] set-up, [3] expansion, [4] level 0 (probe + scoring + sum),
 * [5] evaluation of levels > 0, [6] writing the rows, [7] states visited, [8] rows with as many draws left as their shanten number
 * (their tenpai level is neither built nor evaluated, so [7] holds no level-0 state of theirs).  Measurement only (bench.py
 * `sp_phases`). */
int mj_sp_phase_ticks(MjPool* pool, uint64_t* out9, void* stream);
/* Small-pool schedule of the SP kernel (round 6).  The reference spreads the decisions of a batch over every core and pins nothing
 * (agent/mortal.rs:252-287: rayon par_iter over the batch's states); here a decision row is pinned to one 256-thread workgroup of
 * mj_k_sp, and with few rows per launch the launch lasts as long as its heaviest row.  With the schedule on, a workgroup that finds a
 * row's state graph large (the level it is about to expand has >= min_level1 / min_level2 states) parks the row and a 1,024-thread
 * workgroup of the kernel mj_k_sp_wide [wide_grid of them, one per CU, running beside mj_k_sp] finishes it; results are bit-identical either way.
 * In auto mode the schedule switches itself off for a pool whose two kernels turn out not to overlap (more concurrent streams than hardware
 * queues: the wide workgroups give up after 50 ms, the sweep launch still finishes every parked row, one line on stderr).
 * mode: -1 auto (launches of at most max_rows rows; the default, also settable through MJ_SP_WIDE / MJ_SP_WIDE_MAX_ROWS /
 * MJ_SP_WIDE_GRID / MJ_SP_PROMO_MIN1 / _MIN2), 0 never, 1 every launch.  Arguments <= 0 keep the current value (mode: < -1).
 * The environment is read when the pool is created and applied at its first obs-v4 mj_encode, unless this function was called first:
 * then none of those variables applies to the pool.
 * Call it before the pool's first obs-v4 mj_encode (the spare work areas are sized then); afterwards only mode 0 / the thresholds change. */
int mj_pool_set_sp_schedule(MjPool* pool, int mode, int max_rows, int wide_grid, int min_level1, int min_level2);
/* out[0] launches that ran both kernels, [1] rows parked and finished by mj_k_sp_wide, [2] rows the sweep launch had to take (the two
 * kernels did not overlap), [3] wide workgroups that gave up waiting (same), since the pool was created.  Measurement only. */
int mj_sp_schedule_stats(MjPool* pool, uint64_t* out4, void* stream);

/* Uniform-random legal action per row, counter-based (seed, game id, seat, kan flag, cycle). */
int mj_random_policy(MjPool* pool, int agent, const uint8_t* masks_dev, uint64_t seed, uint64_t cycle,
                     int32_t* actions_dev, void* stream);

/* Tenpai-seeking policy per row (always agari, mostly riichi, shanten-lowering discards read from the encoded obs' discard
 * block, occasional calls), counter-based like mj_random_policy but keyed by the table index.  No reference counterpart:
 * the benchmark's realistic-hand workload and the parity tests' policy (tests/parity_util.py greedy_actions). */
int mj_greedy_policy(MjPool* pool, int agent, const uint8_t* masks_dev, const float* obs_dev, uint64_t seed, uint64_t cycle,
                     int32_t* actions_dev, void* stream);

/* counters: [0] env steps (live tables summed over cycles), [1] games finished, [2] tables in error,
 *           [3] decisions, [4] quick-eval decisions, [5] cycles, [6] SP hash-set overflows (must stay 0) */
int mj_counters(MjPool* pool, uint64_t out[8], void* stream);
/* Final scores [n_games_total][4] and done flags (0 running, 1 finished, 2 aborted on error) to host memory. */
int mj_results(MjPool* pool, int32_t* scores_out, uint8_t* done_out, void* stream);
/* ---- libriichi's Stat (stat.rs:30-126) reduced from packed event logs on the device (kernel: mortal_amd/csrc/mj_stat.hip).
 * One int64 counter per field, in the declaration order of stat.rs:30-126 (= mortal_amd/stat.py STAT_FIELDS): */
#define MJ_STAT_FIELDS 44
enum MjStatField {
    MJ_ST_GAME = 0, MJ_ST_ROUND, MJ_ST_OYA, MJ_ST_POINT, MJ_ST_RANK_1, MJ_ST_RANK_2, MJ_ST_RANK_3, MJ_ST_RANK_4, MJ_ST_TOBI,
    MJ_ST_FUURO, MJ_ST_FUURO_NUM, MJ_ST_FUURO_POINT, MJ_ST_FUURO_AGARI, MJ_ST_FUURO_AGARI_JUN, MJ_ST_FUURO_AGARI_POINT,
    MJ_ST_FUURO_HOUJUU, MJ_ST_AGARI, MJ_ST_AGARI_AS_OYA, MJ_ST_AGARI_JUN, MJ_ST_AGARI_POINT_OYA, MJ_ST_AGARI_POINT_KO,
    MJ_ST_HOUJUU, MJ_ST_HOUJUU_JUN, MJ_ST_HOUJUU_TO_OYA, MJ_ST_HOUJUU_POINT_TO_OYA, MJ_ST_HOUJUU_POINT_TO_KO,
    MJ_ST_RIICHI, MJ_ST_RIICHI_AS_OYA, MJ_ST_RIICHI_JUN, MJ_ST_RIICHI_AGARI, MJ_ST_RIICHI_AGARI_POINT, MJ_ST_RIICHI_AGARI_JUN,
    MJ_ST_RIICHI_HOUJUU, MJ_ST_RIICHI_RYUKYOKU, MJ_ST_RIICHI_POINT, MJ_ST_CHASING_RIICHI, MJ_ST_RIICHI_GOT_CHASED,
    MJ_ST_DAMA_AGARI, MJ_ST_DAMA_AGARI_JUN, MJ_ST_DAMA_AGARI_POINT, MJ_ST_RYUKYOKU, MJ_ST_RYUKYOKU_POINT, MJ_ST_YAKUMAN,
    MJ_ST_NAGASHI_MANGAN
};
/* stat.rs:263-441 Stat::from_game over n_logs packed event logs (LG_* words, the words mj_log_read returns or mortal_amd/mjai_log.py
 * encode_events builds; host arrays; no pool needed, only a device).  Log i = words[off[i] .. off[i + 1]); seats[i] bit s = seat s of
 * log i is counted; groups[i] bit s = which of the two totals that seat goes to.  per_seat rows of seats that are not counted are 0.
 * counts_out = {logs reduced, logs skipped (length 0), malformed logs (the event chain runs past the end of the log or meets an
 * event type outside 1..14; they contribute nothing)}.  A log that stops between two events, in the middle of a kyoku or of a
 * hanchan, is reduced like the reference reduces that prefix.  Synchronous. */
int mj_stat_logs(const uint64_t* words_host, const uint32_t* off_host /* [n_logs + 1] */, int n_logs,
                 const uint8_t* seats_host /* [n_logs] 4-bit masks, NULL = all */, const uint8_t* groups_host /* NULL = 0 */,
                 int64_t* totals_out /* [2][MJ_STAT_FIELDS] */, int64_t* per_seat_out /* NULL or [n_logs][4][MJ_STAT_FIELDS] */,
                 int64_t counts_out[3], void* stream);
/* The same over the pool's own device log, in place: every table whose game has finished (done == 1); running tables and
 * tables in error are skipped and counted.  group bit = agent_of_seat.  Needs mj_pool_enable_log; ordered behind the steps already
 * launched on `stream`; synchronous.  An error in refill mode: a restarted table's log has been rewound (mj_harvest_stat is the route there). */
int mj_pool_stat(MjPool* pool, const uint8_t* seats_host /* [n_tables], NULL = all */, int64_t* totals_out,
                 int64_t* per_seat_out /* NULL or [n_tables][4][MJ_STAT_FIELDS] */, int64_t counts_out[3], void* stream);

/* ---- Grp::load_events (dataset/grp.rs:90-164) reduced from packed event logs on the device (kernel: mortal_amd/csrc/mj_gameplay.hip).
 * Addressing and host arrays as mj_stat_logs.  Per log: n_kyoku_out = its number of start_kyoku events, feat_out[k] = {grand kyoku
 * (grp.rs:135-139), honba, kyotaku, scores[4]} of the k-th as raw integers (the reference's f64 feature is score / 10000., left to the
 * caller: the same f64 division gives the same bits), rank_out = rank_by_player, final_out = final_scores (the last kyoku's scores
 * plus its deltas, minus 1000 per accepted riichi; ranks stable, ties to the lower seat; what a sum below 100,000 lacks goes to
 * first place after ranking).  counts_out = {logs reduced, skipped (length 0: n_kyoku 0), malformed (no start_kyoku, more than
 * max_kyoku of them, an unknown event type or a chain that runs past the end of the log: n_kyoku -1)}; a skipped or malformed
 * log's other outputs are zeros.  Synchronous. */
int mj_grp_logs(const uint64_t* words_host, const uint32_t* off_host /* [n_logs + 1] */, int n_logs, int max_kyoku,
                int32_t* feat_out /* [n_logs][max_kyoku][7] */, int32_t* n_kyoku_out /* [n_logs] */, int32_t* rank_out /* [n_logs][4] */,
                int32_t* final_out /* [n_logs][4] */, int64_t counts_out[3], void* stream);
/* The same over tables [table0, table0 + n) of the pool's own device log, in place; tables are skipped as by mj_pool_stat (running, or
 * in error), a log_len beyond the log's capacity is malformed.  Needs mj_pool_enable_log; an error in refill mode (mj_harvest_grp is the
 * route there); ordered behind the steps already launched; synchronous. */
int mj_pool_grp(MjPool* pool, int table0, int n, int max_kyoku, int32_t* feat_out, int32_t* n_kyoku_out, int32_t* rank_out,
                int32_t* final_out, int64_t counts_out[3], void* stream);
/* Event::augment (mjai/event.rs:187-217) of packed host logs, through the copy kernel of mj_replay_load_pool with MJ_LOAD_AUGMENT and
 * back: addressing as mj_grp_logs, words_out_host as large as words_host (it may be words_host itself).  A log whose chain is a
 * sequence of known events that ends at its end is written, swapped, to its own offsets; a malformed one is copied unchanged.
 * counts_out = {logs done, empty, malformed}.  No header bit is set or cleared, so the call is its own inverse.  Synchronous. */
int mj_augment_logs(const uint64_t* words_host, const uint32_t* off_host /* [n_logs + 1] */, int n_logs,
                    uint64_t* words_out_host /* as words_host */, int64_t counts_out[3] /* done / empty / malformed */, void* stream);

/* ---- Finished games of a pool in refill mode (kernel: mortal_amd/csrc/mj_harvest.hip).  The reference's arena hands each GameResult
 * over as its game finishes (arena/game.rs:291-296) and a GameResult keeps seed, scores and log (arena/result.rs:19-51).  Here a
 * finished table is restarted in the next step and its log rewound; with harvesting enabled that step first copies the finished game
 * -- log words, seed, final scores -- into the pool's active harvest buffer, on the device.  mj_harvest_take detaches the buffer as an
 * MjHarvest; Stat, Grp and the replay loader then run on it like on a pool's log. */
typedef struct MjHarvest MjHarvest;
typedef struct MjHarvestGame {      /* one collected game */
    uint64_t seed_nonce, seed_key;  /* the game's seed (board.rs:99-107) */
    uint64_t first_word;            /* its log = words [first_word, first_word + n_words) of the harvest */
    uint32_t n_words;               /* 0 for a game that ended in error or whose log overflowed: no words are kept */
    uint32_t game_id;
    uint32_t table;
    uint32_t cycle;                 /* the pool's cycle index of the step that collected (and restarted) the table */
    int32_t scores[4];              /* final scores, as mj_results reports them */
    uint8_t err;                    /* the table's error code, 0 = none */
    uint8_t agent_of_seat;
    uint8_t reserved[6];
} MjHarvestGame;                    /* 64 bytes */
/* Allocate the active buffer: room for max_games records and max_words log words (a game takes its word count rounded up to even).
 * Needs mj_pool_enable_log.  May be called before or after mj_pool_set_refill; games are collected only while the refill mode is on.
 * A game that finds the buffer full is dropped and counted, nothing is overwritten, the table is restarted as usual.  Calling it again
 * replaces the buffer (what it held is discarded); max_games 0 turns harvesting off again. */
int mj_pool_enable_harvest(MjPool* pool, uint32_t max_games, uint64_t max_words);
/* out = {games, words reserved, games dropped} in the active buffer right now (behind the steps already launched); one small copy. */
int mj_harvest_pending(MjPool* pool, int64_t out[3], void* stream);
/* Detach the active buffer as *out (which owns it; mj_harvest_destroy frees it) and give the pool a fresh one of the same size: later
 * steps write into the replacement.  Ordered behind the steps already launched, whatever their stream; synchronous.  The records are
 * copied to the host and sorted by (game_id, table): "game i" below is the i-th record of that order.  A table is collected by the step
 * that restarts it, so a game that has finished but has not been restarted yet is not in this take: it is in the next one. */
int mj_harvest_take(MjPool* pool, MjHarvest** out, void* stream);
void mj_harvest_destroy(MjHarvest* h);
/* out = {games, log words of all games, games dropped while this buffer was active, games in error}. */
int mj_harvest_info(const MjHarvest* h, int64_t out[4]);
int mj_harvest_games(const MjHarvest* h, MjHarvestGame* host_out /* [games], sorted */);
/* The words of one game (the words mj_log_read returned for its table before the restart) to host memory, [n_words]. */
int mj_harvest_read(const MjHarvest* h, int game, uint64_t* words_out);
/* mj_pool_stat over the harvest: seats_host [games] (NULL = all), per_seat_out NULL or [games][4][MJ_STAT_FIELDS]; group bit = the
 * record's agent_of_seat; a game in error is counted as skipped.  Synchronous. */
int mj_harvest_stat(const MjHarvest* h, const uint8_t* seats_host, int64_t* totals_out, int64_t* per_seat_out, int64_t counts_out[3],
                    void* stream);
/* mj_pool_grp over games [game0, game0 + n) of the harvest. */
int mj_harvest_grp(const MjHarvest* h, int game0, int n, int max_kyoku, int32_t* feat_out, int32_t* n_kyoku_out, int32_t* rank_out,
                   int32_t* final_out, int64_t counts_out[3], void* stream);
/* mj_replay_load_pool from a harvest: log t of `dst` = game game0 + t, for all dst->n_tables tables; flags = MJ_LOAD_* as there
 * (MJ_LOAD_AUGMENT: the script is suit-swapped on the way; an unknown bit is an error), with MJ_LOAD_DEAL_FROM_SEED the seeds come
 * from the records.  A game in error is skipped.  The destination is built beside dst and moved in last: a failing call leaves dst
 * and the harvest as they were. */
int mj_replay_load_harvest(MjPool* dst, const MjHarvest* h, int game0, const uint8_t* tracked_host /* NULL ok */,
                           int always_include_kan_select, int flags /* MJ_LOAD_* */, int64_t counts_out[3], void* stream);

/* ---- Sample store: the replay buffer of mortal/dataloader.py:45-113 (populate_buffer keeps every obs of a batch of files and
 * shuffles them), kept as records (kernels: mortal_amd/csrc/mj_samples.hip).  The encoders read nothing of a decision but its
 * snapshot record and its row descriptor, so a store keeps those -- about 2 KB per sample where an obs takes 127 to 138 KB -- with the
 * eight int32 of mj_replay_meta, and encodes any list of its samples on demand with the kernels of mj_encode / mj_encode_oracle,
 * bit for bit what they gave when the decision was replayed.  Samples are appended from replay pools (mj_replay_load*) and
 * addressed by index, in the order they were appended.
 * capacity: 1 .. 2^28 - 1 samples (an index takes the table bits of a row descriptor); version: obs version 1..4; batch_rows: rows
 * per encode launch (a larger request is served in chunks; for obs v4 it sizes the SP work areas like a pool of that many tables).
 * NULL + mj_last_error on failure.  A store lives on the device of the lookup tables, like a pool. */
typedef struct MjSamples MjSamples;
MjSamples* mj_samples_create(int64_t capacity, int version, int batch_rows);
void mj_samples_destroy(MjSamples* s);
/* dataset/gameplay.rs:239-443 (one entry per decision of a tracked seat): the rows of agent 0 of replay_pool's last mj_replay_step
 * (mj_rows_count done) become samples count .. count + rows - 1, all of them or none: each row its own copy of its table's record, even
 * where several rows of the step name one table.  meta [1] of a sample is log_base + its table.  Ordered behind the pool's
 * snapshot, whatever its stream.  An error if the pool has no replay script (the label comes from it) or the rows do not fit. */
int mj_samples_append(MjSamples* s, MjPool* replay_pool, int32_t log_base, void* stream);
/* Forget the samples from `count` on (count <= the current count; 0 = clear). */
int mj_samples_truncate(MjSamples* s, int64_t count);
/* out = {count, capacity, device bytes per sample, overflow flags: the encoder's op list | SP hash-set overflows of every encode so
 * far (must stay 0, as mj_counters [6])}; waits for the stream of the last encode. */
int mj_samples_info(const MjSamples* s, int64_t out4[4]);
/* The int32[8] of samples [first, first + n) to host memory: {label, game, seat, kyoku index, turn, shanten, is kan-select row,
 * event index} (mj_replay_meta's, game = log_base + table).  Synchronous. */
int mj_samples_meta(const MjSamples* s, int64_t first, int64_t n, int32_t* meta_host /* [n][8] */, void* stream);
/* agent/mortal.rs:252-287 -> state/obs_repr.rs:126-630 over stored decisions: obs_dev [n][C][34] f32, masks_dev [n][46] u8 of the
 * samples idx_host[0..n) names (a host array; any order, duplicates allowed), as mj_encode wrote them for those rows.  Every index is
 * checked before anything is queued: a refused call writes nothing.  Asynchronous on `stream`; idx_host may go when the call returns. */
int mj_samples_encode(MjSamples* s, const int32_t* idx_host, int n, float* obs_dev, uint8_t* masks_dev, void* stream);
/* dataset/invisible.rs (Invisible::encode) over stored decisions: out_dev [n][mj_oracle_obs_rows][34] f32, every undrawn yama tile
 * listed as mj_encode_oracle does for a replay pool.  Meaningful for samples whose pool was loaded with its walls (MJ_LOAD_DEAL_FROM_SEED). */
int mj_samples_encode_oracle(MjSamples* s, const int32_t* idx_host, int n, float* out_dev, void* stream);

/* First table in error: returns its error code (>0) and index, or 0. */
int mj_pool_first_error(MjPool* pool, int* table_out, void* stream);

/* Debug/test: copy one table's state (struct TableOne, mortal_amd/csrc/mj_state.h) to host memory. */
int mj_debug_table(MjPool* pool, int table, void* out, size_t out_size, void* stream);
size_t mj_debug_table_size(void);
/* "name:elem_size:count:offset;..." describing the struct returned by mj_debug_table. */
const char* mj_debug_layout(void);
int mj_obs_rows(int version);

/* Debug/test: the pure rule functions of the device code applied to explicit inputs, one device thread per query (no pool
 * needed, only mj_tables_upload).  This is how the reference's own known-answer tests reach the HIP code
 * (algo/shanten.rs:158-201, algo/agari.rs:920-1379, algo/point.rs:121-153; tests/test_gpu_kats.py).
 *   op 0 calc_shanten(tehai, len_div3)                       -> r0 = shanten            (algo/shanten.rs:139-150)
 *   op 1 AgariCalculator::search_yakus                        -> r0 = kind (0 none, 1 fu/han, 2 yakuman), r1 = fu, r2 = han or
 *                                                                yakuman count           (algo/agari.rs:260-288)
 *   op 2 AgariCalculator::has_yaku                            -> r0 = 0 / 1
 *   op 3 AgariCalculator::agari(additional_hans, doras)       -> r0..r2 as op 1; r3 = 1   (algo/agari.rs:228-258)
 *        followed by Agari::point(arg0 = is_oya)              -> p0 = ron, p1 = tsumo_ko, p2 = tsumo_oya
 *   op 4 check_ankan_after_riichi(tehai incl. the drawn tile, len_div3, arg0 = tile), non-strict -> r0 (algo/agari.rs:854-912)
 *   op 5 Point::calc(arg0 = is_oya, arg1 = fu, arg2 = han)    -> p0..p2                   (algo/point.rs:13-112)
 *   op 6 the wall shuffle's u32 division (x = tehai[0..3] little endian, n = arg0 in 1..136) -> r0 = x / n, r1 = x % n
 *        (the `chunk % next_n`, `chunk /= next_n` steps of rand 0.9.1's IncreasingUniform behind arena/board.rs:107-109)
 * Queries and results are host arrays. */
typedef struct MjAlgoQuery {
    uint8_t tehai[34];                                  /* tile counts, red fives counted as fives (34-tile form) */
    uint8_t chis[4], pons[4], minkans[4], ankans[4];    /* deaka'd tile ids (lowest tile of a chi) */
    uint8_t n_chis, n_pons, n_minkans, n_ankans;
    uint8_t len_div3, is_menzen, bakaze, jikaze, winning_tile, is_ron, additional_hans, doras;
    uint8_t op, arg0, arg1, arg2;
    uint8_t pad[6];
} MjAlgoQuery;                                          /* 72 bytes */
typedef struct MjAlgoResult {
    int32_t r0, r1, r2, r3, p0, p1, p2, p3;
} MjAlgoResult;
int mj_algo_query(const MjAlgoQuery* queries_host, int n, MjAlgoResult* results_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
