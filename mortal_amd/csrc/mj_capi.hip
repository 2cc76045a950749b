// C-ABI host side (include/mortal_amd.h): pool life-cycle and kernel launches.  One translation unit for the whole
// library; the kernels live in mj_step.hip / mj_replay.hip / mj_encode.hip / mj_sp.hip / mj_stat.hip / mj_gameplay.hip / mj_harvest.hip / mj_samples.hip
// (mj_log.h: what the kernels over packed logs share).
// Host float math below builds bit-exact LUTs: compile with -ffp-contract=off.
// Ownership: whatever the host takes from the HIP runtime is held by an owner of mj_host.h and released by its destructor; a call that
// returns an error leaves the pool as it was before the call (a fallible call builds into locals and moves them in as its last step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../../include/mortal_amd.h"
#include "mj_host.h"
#include "mj_step.hip"
#include "mj_replay.hip"
#include "mj_encode.hip"
#include "mj_sp.hip"
#include "mj_stat.hip"
#include "mj_gameplay.hip"
#include "mj_harvest.hip"
#include "mj_samples.hip"

static_assert(sizeof(MjAlgoQuery) == 72, "MjAlgoQuery layout");
// include/mortal_amd.h mj_algo_query: one thread per query, the same device functions the step / encode / SP kernels call
__global__ __launch_bounds__(64) void mj_k_algo_query(const MjAlgoQuery* q, int n, MjAlgoResult* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const MjAlgoQuery Q = q[i];
    MjAlgoResult R = {0, 0, 0, 0, 0, 0, 0, 0};
    Hand h = {0, 0};
    for (int t = 0; t < 34; t++)
        for (int c = 0; c < (int)Q.tehai[t] && c < 4; c++) h.inc(t);
    AgariIn in;
    in.tehai = h;
    in.m.chis = in.m.pons = in.m.minkans = in.m.ankans = 0;
    for (int k = 0; k < 4; k++) {
        melds_put(in.m.chis, k, Q.chis[k]);
        melds_put(in.m.pons, k, Q.pons[k]);
        melds_put(in.m.minkans, k, Q.minkans[k]);
        melds_put(in.m.ankans, k, Q.ankans[k]);
    }
    in.m.n_chis = Q.n_chis;
    in.m.n_pons = Q.n_pons;
    in.m.n_minkans = Q.n_minkans;
    in.m.n_ankans = Q.n_ankans;
    in.is_menzen = Q.is_menzen != 0;
    in.bakaze = Q.bakaze;
    in.jikaze = Q.jikaze;
    in.winning_tile = Q.winning_tile;
    in.is_ron = Q.is_ron != 0;
    auto put = [&](const Agari& a) { R.r0 = a.kind; R.r1 = a.fu; R.r2 = a.han; };
    auto put_point = [&](const Point& p) { R.p0 = p.ron; R.p1 = p.tsumo_ko; R.p2 = p.tsumo_oya; };
    switch (Q.op) {
        case 0: R.r0 = calc_all(c_mj_tables, h, Q.len_div3); break;
        case 1: put(agari_search(c_mj_tables, in, false)); break;
        case 2: R.r0 = agari_search(c_mj_tables, in, true).kind != 0; break;
        case 3: {
            const Agari a = agari_full(c_mj_tables, in, Q.additional_hans, Q.doras);
            put(a);
            R.r3 = 1;
            if (a.kind) put_point(agari_point(a, Q.arg0 != 0));
            break;
        }
        case 4: R.r0 = check_ankan_after_riichi(c_mj_tables, h, Q.len_div3, Q.arg0); break;
        case 5: put_point(point_calc(Q.arg0 != 0, Q.arg1, Q.arg2)); break;
        case 6: {  // the shuffle's division by multiply-high (mj_deal.h: deal_divmod), x = tehai[0..3] little endian, n = arg0
            const u32 x = (u32)Q.tehai[0] | ((u32)Q.tehai[1] << 8) | ((u32)Q.tehai[2] << 16) | ((u32)Q.tehai[3] << 24);
            u32 qq = 0, rr = 0;
            if (Q.arg0 >= 1 && Q.arg0 <= 136) deal_divmod(x, (u32)Q.arg0, qq, rr);
            R.r0 = (int32_t)qq;
            R.r1 = (int32_t)rr;
            break;
        }
        default: R.r3 = -1; break;
    }
    out[i] = R;
}

namespace {

struct DevTables {
    bool ready = false;
    int device = -1;  // the HIP device the tables (and the __constant__ copy of their pointers) live on
    MjTablesDev dev{};
    MjGatherEnt* gather = nullptr;
    int n_gather = 0;
    int gather_chunk[SNAP_NCH + 1] = {0};  // first gather entry of each record chunk (mj_k_snapshot)
    float *decay = nullptr, *rbf_score = nullptr, *rbf_6 = nullptr, *rbf_12 = nullptr, *rbf_23 = nullptr;
} g_tables;

template <class T> int upload(const std::vector<T>& v, T** out) {
    HIP_OK(hipMalloc(out, v.size() * sizeof(T)));
    HIP_OK(hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// device copy of a host array of one mj_stat_logs / mj_pool_stat call (an empty one still gets an address)
template <class T> int stat_upload(DevBuf<T>& b, const T* src, size_t count, hipStream_t s) {
    if (b.alloc(std::max(count, 8 / sizeof(T)))) return -1;
    if (count) HIP_OK(hipMemcpyAsync(b.get(), src, count * sizeof(T), hipMemcpyHostToDevice, s));
    return 0;
}

// obs_repr.rs:79-90 with f32 arithmetic in the reference's order
std::vector<float> build_rbf(int n_max, int cap, int intervals) {
    std::vector<float> out((size_t)n_max * (intervals - 1));
    float interval_size = (float)cap / (float)intervals;
    for (int n = 0; n < n_max; n++)
        for (int i = 1; i < intervals; i++) {
            float x = (float)n;
            float mu = (float)i * interval_size;
            float sigma = interval_size;
            float d = x - mu;
            out[(size_t)n * (intervals - 1) + i - 1] = expf(-(d * d) / (2.f * (sigma * sigma)));
        }
    return out;
}

size_t enc_lds_bytes(int version) {
    int C = enc_rows_written(version);
    int tile_rows = ((C + ENC_PASSES - 1) / ENC_PASSES + 1) & ~1;
    return (size_t)tile_rows * 34 * 4 + ((sizeof(TableOne) + 15) & ~(size_t)15) + sizeof(EncDerived);
}

// The library's environment switches (diagnostics and tests; tools/README.md), read once per pool by mj_pool_create.  The SP
// schedule's switches apply at the pool's first obs-v4 encode unless mj_pool_set_sp_schedule was called.
struct PoolKnobs {
    // MJ_SP_GRID caps mj_k_sp's workgroups (tests: few workgroups, many rows each); MJ_SP_WIDE (0 never / 1 every launch / unset: auto),
    // MJ_SP_WIDE_MAX_ROWS, MJ_SP_WIDE_GRID, MJ_SP_PROMO_MIN1 / _MIN2 (the level sizes that park a row): mj_pool_set_sp_schedule's values
    std::optional<int> sp_grid, sp_wide, sp_wide_max_rows, sp_wide_grid, sp_promo_min1, sp_promo_min2;
    bool sp_wide_serial = false;    // MJ_SP_WIDE_SERIAL: the schedule's three launches one after the other (always in the emulator)
    bool sp_wide_all_rows = false;  // MJ_SP_WIDE_ALL_ROWS (tests, serial only): the wide kernel alone first, it takes every row
    bool sp_prof = false;           // MJ_SP_PROF: mj_k_sp's phase / pass timers, printed by mj_counters
};

PoolKnobs read_knobs() {
    auto num = [](const char* name) { const char* v = getenv(name); return v ? std::optional<int>(atoi(v)) : std::nullopt; };
    PoolKnobs K;
    K.sp_grid = num("MJ_SP_GRID");
    K.sp_wide = num("MJ_SP_WIDE");
    K.sp_wide_max_rows = num("MJ_SP_WIDE_MAX_ROWS");
    K.sp_wide_grid = num("MJ_SP_WIDE_GRID");
    K.sp_promo_min1 = num("MJ_SP_PROMO_MIN1");
    K.sp_promo_min2 = num("MJ_SP_PROMO_MIN2");
#ifdef MJ_EMU
    K.sp_wide_serial = true;  // (the emulator runs a launch to completion)
#else
    K.sp_wide_serial = getenv("MJ_SP_WIDE_SERIAL") != nullptr;
#endif
    K.sp_wide_all_rows = getenv("MJ_SP_WIDE_ALL_ROWS") != nullptr;
    K.sp_prof = getenv("MJ_SP_PROF") != nullptr;
    return K;
}

// HIP event pairs around timed launches, owned by a pool: pairs[0, n_pending) wait for collect(), the rest are free.  A launch
// that fails between begin() and end() leaves its pair free.
struct EventTimer {
    std::vector<std::pair<Event, Event>> pairs;
    size_t n_pending = 0;
    int begin(hipStream_t s) {
        if (n_pending == pairs.size()) {
            Event a, b;
            if (a.create() || b.create()) return -1;
            pairs.emplace_back(std::move(a), std::move(b));
        }
        HIP_OK(hipEventRecord(pairs[n_pending].first.get(), s));
        return 0;
    }
    int end(hipStream_t s) {
        HIP_OK(hipEventRecord(pairs[n_pending++].second.get(), s));
        return 0;
    }
    void collect(double* total_ms, int64_t* launches) {  // the launches timed since the last call; their pairs become free
        double tot = 0;
        for (size_t i = 0; i < n_pending; i++) {
            hipEventSynchronize(pairs[i].second.get());
            float ms = 0;
            hipEventElapsedTime(&ms, pairs[i].first.get(), pairs[i].second.get());
            tot += ms;
        }
        if (total_ms) *total_ms = tot;
        if (launches) *launches = (int64_t)n_pending;
        n_pending = 0;
    }
};

struct SpResources {  // built by sp_setup, moved into the pool whole
    DevBuf<SpWork> work;        // grid areas (one per workgroup of mj_k_sp) + spare + wide_areas
    int grid = 0;               // mj_k_sp's largest grid
    int spare = 0;              // spare work areas = promotions per launch (small pools: mj_sp.hip "promotion"; 0 = this pool never promotes)
    int wide_areas = 0;         // work areas of mj_k_sp_wide's own workgroups (= its largest grid)
    DevBuf<int> queue;          // [0] row queue head, [1..8] / [9..16] class counts / cursors of the row sort, [SP_Q_TAIL] head of the tail
    DevBuf<uint32_t> order;     // [max_rows] queue position -> row
    DevBuf<uint8_t> cls;        // [max_rows] cost class of a row
    DevBuf<unsigned long long> err;     // [SP_ERR_WORDS] counter words (mj_sp.hip SpErrWord)
    Stream stream2;                     // mj_k_sp_promo's stream while mj_k_sp_wide runs on the caller's (spare > 0)
    Event ev_fork, ev_join;
    PinnedBuf<unsigned long long> gaveup_host;  // the device's count of wide workgroups that gave up waiting, copied behind every sweep
};

struct ReplayBufs {  // log replay (dataset loader): built by mj_replay_load, moved into the pool whole
    DevBuf<uint64_t> script;
    DevBuf<uint32_t> off, cursor, ev_index;
    DevBuf<uint8_t> kyoku, tracked;
    DevBuf<int32_t> label, kan_label;
    int always_kan = 1;
};

struct HarvestBuf {  // a harvest buffer (mj_harvest.hip): the pool's active one, or the one an MjHarvest took with it
    DevBuf<MjHarvestGame> games;
    DevBuf<uint64_t> words;
    DevBuf<unsigned long long> cursors;  // [HV_CURSORS]
    uint64_t max_games = 0, max_words = 0;
    int alloc(uint64_t n_games, uint64_t n_words, hipStream_t s) {  // empty, its cursors zeroed on s
        if (games.alloc(n_games) || words.alloc(n_words + 2) || cursors.alloc(HV_CURSORS)) return -1;
        HIP_OK(hipMemsetAsync(cursors.get(), 0, HV_CURSORS * sizeof(unsigned long long), s));
        max_games = n_games, max_words = n_words;
        return 0;
    }
};

std::vector<MjGatherEnt> build_gather() {
    std::vector<MjGatherEnt> v;
#define MJ_X_GATHER(type, name, dims, count)                                                         \
    for (int k = 0; k < (count); k++)                                                                \
        v.push_back({(uint32_t)(offsetof(TableBlock, name) + (size_t)k * MJ_LANES * sizeof(type)),   \
                     (uint16_t)(offsetof(TableOne, name) + (size_t)k * sizeof(type)), (uint16_t)sizeof(type)});
    MJ_FIELDS(MJ_X_GATHER)
#undef MJ_X_GATHER
    return v;
}

}  // namespace

struct MjPool {
    int n_tables = 0, n_blocks = 0, deal_algo = 0, max_rows = 0;
    ReplayBufs rp;
    bool rp_active = false;    // replay mode: the invisible obs lists every undrawn yama tile
    DevBuf<uint64_t> log;      // optional event log [n_tables][log_cap]
    DevBuf<uint32_t> log_len;
    uint32_t log_cap = 0;
    int version[2] = {4, 4};  // obs version per agent (engine.version, agent/mortal.rs:57)
    DevBuf<TableBlock> blocks;
    DevBuf<uint32_t> rows[2];
    DevBuf<int> n_rows_dev, block_rows;
    DevBuf<TableOne> snap;
    PoolKnobs knobs;
    SpResources sp;                 // allocated at the first obs-v4 encode (sp_setup)
    int sp_wide_mode = -1;          // -1 auto (launches of at most sp_wide_max_rows rows), 0 never, 1 always
    int sp_wide_max_rows = 20000, sp_wide_grid = 0, sp_promo_min[4] = {0, 0, 0, 0};  // grid / thresholds 0 = by the launch's row count (sp_launch)
    uint64_t sp_hybrid_launches = 0;
    bool sp_wide_off = false;       // the two kernels did not overlap on this system: the schedule switched itself off (see sp_launch)
    bool sp_sched_set = false;      // mj_pool_set_sp_schedule was called: the environment does not override it
    DevBuf<int> enc_flag;           // [1] an encoder op list overflowed (reported with the SP overflows)
    PinnedBuf<int> n_rows_host;
    Event ev_rows;  // recorded right after the row counts' copy: mj_rows_count waits for it, not for the snapshot behind it
    Event ev_snap;  // recorded after mj_k_snapshot: a reader of P->snap on ANOTHER stream than the step's waits for it
    hipStream_t step_stream = nullptr;  // the stream the last mj_step / mj_table_* launched on
    DevBuf<unsigned long long> counters;
    DevBuf<int> final_scores;
    DevBuf<uint8_t> final_done;
    int n_games_total = 0;
    int enable_quick_eval[2] = {1, 1};
    int enable_agari_guard[2] = {0, 0};
    uint64_t refill_stride = 0;
    uint32_t start_stagger = 0;
    HarvestBuf hv;                  // active harvest buffer (mj_pool_enable_harvest); filled by mj_k_harvest while the refill mode is on
    uint64_t cycles = 0;
    int last_rows[2] = {0, 0};
    bool rows_valid = false;
    // encode timing (mj_encode_timing; the SP launches are timed with it)
    bool timing = false;
    EventTimer enc_timer, sp_timer;
};

// Host image of a pool at the start of play: zeroed tables, the padding lanes of the last block inactive, the seeds if given
static std::vector<TableBlock> fresh_blocks(const MjPool* P, const uint64_t* nonces, const uint64_t* keys) {
    std::vector<TableBlock> host(P->n_blocks);
    memset(host.data(), 0, host.size() * sizeof(TableBlock));
    for (int t = P->n_tables; t < P->n_blocks * MJ_LANES; t++) host[t >> 6].flags[t & 63] = TF_INACTIVE | TF_DONE | TF_ENDED;
    if (nonces && keys)
        for (int t = 0; t < P->n_tables; t++) {
            host[t >> 6].seed_nonce[t & 63] = nonces[t];
            host[t >> 6].seed_key[t & 63] = keys[t];
        }
    return host;
}

extern "C" {

const char* mj_last_error(void) { return g_err.c_str(); }
int mj_abi_version(void) { return 1; }
int mj_obs_rows(int version) { return version == 1 ? 938 : version == 2 ? 942 : version == 3 ? 934 : version == 4 ? 1012 : -1; }
size_t mj_debug_table_size(void) { return sizeof(TableOne); }
int mj_algo_query(const MjAlgoQuery* queries_host, int n, MjAlgoResult* results_host, void* stream) {
    if (!g_tables.ready) return fail("mj_tables_upload has not been called");
    if (n <= 0) return 0;
    if (!queries_host || !results_host) return fail("null query / result buffer");
    DevBuf<MjAlgoQuery> bq;
    DevBuf<MjAlgoResult> br;
    hipStream_t s = (hipStream_t)stream;
    if (bq.alloc(n) || br.alloc(n)) return -1;
    MjAlgoQuery* dq = bq.get();
    MjAlgoResult* dr = br.get();
    HIP_OK(hipMemcpyAsync(dq, queries_host, (size_t)n * sizeof(MjAlgoQuery), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(mj_k_algo_query, dim3((n + 63) / 64), dim3(64), 0, s, dq, n, dr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(results_host, dr, (size_t)n * sizeof(MjAlgoResult), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}
// "name:elem_size:count:offset;..." of struct TableOne, so a host tool can decode mj_debug_table() generically
const char* mj_debug_layout(void) {
    static std::string s;
    if (s.empty()) {
#define MJ_X_LAYOUT(type, name, dims, count) \
    s += std::string(#name) + ":" + std::to_string(sizeof(type)) + ":" + std::to_string(count) + ":" + \
         std::to_string(offsetof(TableOne, name)) + ";";
        MJ_FIELDS(MJ_X_LAYOUT)
#undef MJ_X_LAYOUT
    }
    return s.c_str();
}

int mj_tables_upload(const void* payload, size_t size) {
    if (g_tables.ready) return 0;
    const uint8_t* p = (const uint8_t*)payload;
    if (size < 16 || memcmp(p, "MJT1", 4) != 0) return fail("bad table payload");
    uint32_t ns, nj, na;
    memcpy(&ns, p + 4, 4);
    memcpy(&nj, p + 8, 4);
    memcpy(&na, p + 12, 4);
    if (size != 16 + (size_t)ns * 5 + (size_t)nj * 5 + (size_t)na * 24) return fail("bad table payload size");
    auto rows = [](const uint8_t* b, uint32_t n) {
        std::vector<uint64_t> v(n);
        for (uint32_t i = 0; i < n; i++) {
            uint64_t r = 0;
            for (int k = 0; k < 5; k++) r |= (uint64_t)b[(size_t)i * 5 + k] << (8 * k);
            v[i] = r;
        }
        return v;
    };
    std::vector<uint64_t> suhai = rows(p + 16, ns), jihai = rows(p + 16 + (size_t)ns * 5, nj);
    const uint8_t* ag = p + 16 + (size_t)ns * 5 + (size_t)nj * 5;
    std::vector<uint32_t> keys(na), divs((size_t)na * 5);
    for (uint32_t i = 0; i < na; i++) {
        uint32_t rec[6];
        memcpy(rec, ag + (size_t)i * 24, 24);
        keys[i] = rec[0];
        for (int k = 0; k < 5; k++) divs[(size_t)i * 5 + k] = rec[1 + k];
    }
    std::vector<uint64_t> ahash(32768, 0);
    for (uint32_t i = 0; i < na; i++) {
        uint32_t pos = (keys[i] * 0x9E3779B1u) >> 17;
        while (ahash[pos]) pos = (pos + 1) & 32767;
        ahash[pos] = ((uint64_t)keys[i] << 32) | (uint64_t)(i + 1);
    }
    uint64_t *d_s, *d_j, *d_h;
    uint32_t *d_k, *d_d;
    if (upload(suhai, &d_s) || upload(jihai, &d_j) || upload(keys, &d_k) || upload(divs, &d_d) || upload(ahash, &d_h)) return -1;
    g_tables.dev = {d_s, ns, d_j, nj, d_k, d_h, d_d, na};
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(c_mj_tables), &g_tables.dev, sizeof(MjTablesDev)));
    {   // table-id shanten (mj_sptab.h): row ids, merge closure, optimal-entry table, per-key wait / keep masks
        SpTabHost H;
        if (!sp_tab_build(suhai.data(), ns, jihai.data(), nj, H)) return fail("sp_tab_build: " + H.error);
        u8 *d_id, *d_m;
        SpRec *d_o, *d_wk;
        if (upload(H.id, &d_id) || upload(H.mrg, &d_m) || upload(H.opt, &d_o) || upload(H.wk, &d_wk)) return -1;
        SpTabDev st{d_id, d_m, d_o, d_wk, ns, nj, H.zero_id};
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(c_sp_tab), &st, sizeof(SpTabDev)));
        std::vector<float> nt((size_t)SP_NT_ROWS * SP_NT_ROWS * SP_NT_STRIDE);  // not_tsumo rows of every wall size (mj_sp.hip)
        sp_not_tsumo_build(nt.data());
        float* d_nt;
        if (upload(nt, &d_nt)) return -1;
        const float* d_ntc = d_nt;
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(c_sp_nt), &d_ntc, sizeof d_ntc));
    }
    auto g = build_gather();
    g_tables.n_gather = (int)g.size();
    for (int c = 0, k = 0; c <= SNAP_NCH; c++) {  // entries are in field order = ascending dst_off
        while (k < (int)g.size() && (int)g[k].dst_off < c * SNAP_CH) k++;
        g_tables.gather_chunk[c] = c == SNAP_NCH ? (int)g.size() : k;
    }
    for (size_t k = 1; k < g.size(); k++)
        if (g[k].dst_off < g[k - 1].dst_off) return fail("gather list not in record order");
    if (upload(g, &g_tables.gather)) return -1;
    std::vector<float> decay(64);
    for (int k = 0; k < 64; k++) decay[k] = expf(-0.2f * (float)k);  // obs_repr.rs:228,266
    if (upload(decay, &g_tables.decay) || upload(build_rbf(4096, 500, 10), &g_tables.rbf_score) ||
        upload(build_rbf(256, 6, 3), &g_tables.rbf_6) || upload(build_rbf(256, 12, 3), &g_tables.rbf_12) ||
        upload(build_rbf(256, 23, 4), &g_tables.rbf_23))
        return -1;
    HIP_OK(hipGetDevice(&g_tables.device));
    // ready only after c_mj_tables AND c_sp_tab / c_sp_nt are on the device: since round 5 the step kernel of EVERY obs version walks the
    // table-id sets (mj_rules.h: update_shanten_discards / update_waits_and_furiten), and no pool can be created before this flag is set
    g_tables.ready = true;
    return 0;
}

MjPool* mj_pool_create(int n_tables, int version, int deal_algo, int max_rows) {
    if (!g_tables.ready) {
        fail("mj_tables_upload has not been called");
        return nullptr;
    }
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != g_tables.device) {  // one process per GPU: pools live where the tables are
        fail("the lookup tables were uploaded to HIP device " + std::to_string(g_tables.device) + ", the current device is " +
             std::to_string(cur) + ": use one process per GPU (tables and pools of a process share one device)");
        return nullptr;
    }
    if (n_tables <= 0 || mj_obs_rows(version) < 0) {
        fail("bad n_tables / version");
        return nullptr;
    }
    std::unique_ptr<MjPool> P(new MjPool);
    P->knobs = read_knobs();
    P->n_tables = n_tables;
    P->n_blocks = (n_tables + MJ_LANES - 1) / MJ_LANES;
    P->version[0] = P->version[1] = version;
    P->deal_algo = deal_algo;
    P->max_rows = max_rows > 0 ? max_rows : 8 * n_tables;
    if (P->blocks.alloc(P->n_blocks) || P->rows[0].alloc(P->max_rows) || P->rows[1].alloc(P->max_rows) || P->n_rows_dev.alloc(2) ||
        P->block_rows.alloc((size_t)P->n_blocks * 2) || P->snap.alloc((size_t)P->n_blocks * MJ_LANES) || P->n_rows_host.alloc(2) ||
        P->counters.alloc(8) || P->enc_flag.alloc(1))
        return nullptr;  // (~MjPool releases what was allocated)
    if (hipMemset(P->enc_flag.get(), 0, sizeof(int)) != hipSuccess) return fail("hipMemset of the encoder's overflow flag failed"), nullptr;
    hipMemset(P->blocks.get(), 0, (size_t)P->n_blocks * sizeof(TableBlock));
    for (int v = 1; v <= 4; v++) {
        const void* fn = v == 1 ? (const void*)mj_k_encode<1> : v == 2 ? (const void*)mj_k_encode<2>
                       : v == 3 ? (const void*)mj_k_encode<3> : (const void*)mj_k_encode<4>;
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)enc_lds_bytes(v));
    }
    return P.release();
}

void mj_pool_destroy(MjPool* P) { delete P; }

int mj_pool_reset(MjPool* P, const uint64_t* nonces, const uint64_t* keys, const uint32_t* game_ids,
                  const uint8_t* agent_of_seat, int n_games_total) {
    if (!P) return fail("null pool");
    std::vector<TableBlock> host = fresh_blocks(P, nonces, keys);
    for (int t = 0; t < P->n_tables; t++) {
        TableBlock& B = host[t >> 6];
        int l = t & 63;
        B.game_id[l] = game_ids ? game_ids[t] : (uint32_t)t;
        B.agent_of_seat[l] = agent_of_seat ? agent_of_seat[t] : 0;
        for (int i = 0; i < 4; i++) B.scores[i][l] = 25000;  // BatchGame::tenhou_hanchan (game.rs:222-228)
    }
    const int n_games = n_games_total > 0 ? n_games_total : P->n_tables;
    DevBuf<int> final_scores;
    DevBuf<uint8_t> final_done;
    if (final_scores.alloc((size_t)n_games * 4) || final_done.alloc(n_games)) return -1;
    HIP_OK(hipMemset(final_scores.get(), 0, (size_t)n_games * 4 * sizeof(int)));
    HIP_OK(hipMemset(final_done.get(), 0, (size_t)n_games));
    HIP_OK(hipMemcpy(P->blocks.get(), host.data(), host.size() * sizeof(TableBlock), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(P->counters.get(), 0, 8 * sizeof(unsigned long long)));
    if (P->log_len) HIP_OK(hipMemset(P->log_len.get(), 0, (size_t)P->n_tables * sizeof(uint32_t)));
    P->final_scores = std::move(final_scores);  // (the previous pair goes with the locals)
    P->final_done = std::move(final_done);
    P->n_games_total = n_games;
    P->rp_active = false;
    P->cycles = 0;
    P->start_stagger = 0;
    P->rows_valid = false;
    return 0;
}

int mj_pool_enable_log(MjPool* P, uint32_t words_per_table) {
    if (!P) return fail("null pool");
    // The one exception to "an error leaves the pool as it was": the log may take a gigabyte, so the old one goes first and a failure
    // leaves the log disabled.
    P->log.reset();
    P->log_len.reset();
    P->log_cap = 0;
    if (words_per_table == 0) return 0;
    DevBuf<uint64_t> log;
    DevBuf<uint32_t> log_len;
    if (log.alloc((size_t)P->n_tables * words_per_table) || log_len.alloc(P->n_tables)) return -1;
    HIP_OK(hipMemset(log_len.get(), 0, (size_t)P->n_tables * sizeof(uint32_t)));
    P->log = std::move(log);
    P->log_len = std::move(log_len);
    P->log_cap = words_per_table;
    return 0;
}
int mj_log_lengths(MjPool* P, uint32_t* len_out, void* stream) {
    if (!P || !P->log) return fail("event log is not enabled");
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    HIP_OK(hipMemcpy(len_out, P->log_len.get(), (size_t)P->n_tables * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
int mj_log_read(MjPool* P, int table0, int n, uint64_t* words_out, void* stream) {
    if (!P || !P->log) return fail("event log is not enabled");
    if (table0 < 0 || n < 0 || table0 + n > P->n_tables) return fail("table range out of bounds");
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    HIP_OK(hipMemcpy(words_out, P->log.get() + (size_t)table0 * P->log_cap, (size_t)n * P->log_cap * sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
    return 0;
}

int mj_pool_configure(MjPool* P, int agent, int version, int enable_quick_eval, int enable_guard) {
    if (!P || agent < 0 || agent > 1) return fail("bad agent");
    if (version != 0) {
        if (mj_obs_rows(version) < 0) return fail("bad obs version");
        P->version[agent] = version;
    }
    P->enable_quick_eval[agent] = enable_quick_eval;
    P->enable_agari_guard[agent] = enable_guard;
    return 0;
}
int mj_pool_set_refill(MjPool* P, uint64_t stride) {
    if (!P) return fail("null pool");
    P->refill_stride = stride;
    return 0;
}

int mj_pool_set_start_stagger(MjPool* P, uint32_t cycles, void* stream) {
    if (!P) return fail("null pool");
    if (P->cycles != 0) return fail("mj_pool_set_start_stagger: call it right after mj_pool_reset, before the first mj_step");
    if (cycles && !P->refill_stride) return fail("mj_pool_set_start_stagger needs the refill mode (mj_pool_set_refill)");
    if (!cycles && P->start_stagger) return fail("mj_pool_set_start_stagger(0) after the tables were parked: reset the pool instead");
    P->start_stagger = cycles;
    if (cycles) hipLaunchKernelGGL(mj_k_park, dim3(P->n_blocks), dim3(64), 0, (hipStream_t)stream, P->blocks.get(), P->n_tables);
    HIP_OK(hipGetLastError());
    return 0;
}

static int launch_rows(MjPool* P, hipStream_t s);
// mj_rows_count returns as soon as the row counts are on the host; mj_k_snapshot, queued behind their copy, may still be running.  A
// reader of the snapshot records on the SAME stream is ordered behind it by the stream; one on another stream waits for ev_snap.
static int wait_snapshot(MjPool* P, hipStream_t s) {
    if (P->ev_snap && s != P->step_stream) HIP_OK(hipStreamWaitEvent(s, P->ev_snap.get(), 0));
    return 0;
}
int mj_step(MjPool* P, const int32_t* a0, const int32_t* a1, void* stream) {
    return mj_step_q(P, a0, a1, nullptr, nullptr, stream);
}
int mj_step_q(MjPool* P, const int32_t* a0, const int32_t* a1, const float* q0, const float* q1, void* stream) {
    return mj_step_ev(P, a0, a1, q0, q1, nullptr, nullptr, stream);
}
int mj_step_ev(MjPool* P, const int32_t* a0, const int32_t* a1, const float* q0, const float* q1, const uint64_t* ev0,
               const uint64_t* ev1, void* stream) {
    if (!P) return fail("null pool");
    if ((P->enable_agari_guard[0] && a0 && !q0) || (P->enable_agari_guard[1] && a1 && !q1))
        return fail("enable_rule_based_agari_guard needs the q-values of the batch (mj_step_q)");
    hipStream_t s = (hipStream_t)stream;
    StepParams sp;
    sp.blocks = P->blocks.get();
    sp.n_tables = P->n_tables;
    sp.tables = g_tables.dev;
    sp.actions[0] = a0;
    sp.actions[1] = a1;
    sp.q_values[0] = q0;
    sp.q_values[1] = q1;
    sp.reactions[0] = ev0;
    sp.reactions[1] = ev1;
    sp.log = P->log.get();
    sp.log_len = P->log_len.get();
    sp.log_cap = P->log_cap;
    sp.cycle = (uint32_t)P->cycles;
    sp.deal_algo = P->deal_algo;
    for (int a = 0; a < 2; a++) {
        sp.enable_quick_eval[a] = P->enable_quick_eval[a];
        sp.enable_agari_guard[a] = P->enable_agari_guard[a];
    }
    sp.game_length = 8;
    sp.refill = P->refill_stride != 0;
    sp.refill_stride = P->refill_stride;
    sp.start_stagger = P->start_stagger;
    sp.counters = P->counters.get();
    sp.final_scores = P->final_scores.get();
    sp.final_done = P->final_done.get();
    sp.n_games_total = P->n_games_total;
    sp.block_rows = P->block_rows.get();
    if (sp.refill && P->hv.games && P->log) {  // what mj_k_refill is about to rewind goes to the harvest buffer first
        const HarvestParams hp = {P->blocks.get(), P->n_tables, sp.cycle, sp.start_stagger, P->log.get(), P->log_len.get(), P->log_cap,
                                  P->hv.games.get(), P->hv.words.get(), P->hv.cursors.get(), P->hv.max_games, P->hv.max_words};
        hipLaunchKernelGGL(mj_k_harvest, dim3(P->n_blocks), dim3(64), 0, s, hp);
    }
    if (sp.refill) hipLaunchKernelGGL(mj_k_refill, dim3(P->n_blocks), dim3(64), 0, s, sp);
    hipLaunchKernelGGL(mj_k_step, dim3(P->n_blocks), dim3(MJ_LANES), 0, s, sp);
    return launch_rows(P, s);
}
static int launch_rows(MjPool* P, hipStream_t s) {
    RowsParams rp;
    rp.blocks = P->blocks.get();
    rp.n_blocks = P->n_blocks;
    rp.block_rows = P->block_rows.get();
    rp.rows[0] = P->rows[0].get();
    rp.rows[1] = P->rows[1].get();
    rp.n_rows_out = P->n_rows_dev.get();
    rp.max_rows[0] = rp.max_rows[1] = P->max_rows;
    hipLaunchKernelGGL(mj_k_scan, dim3(1), dim3(1024), 0, s, rp);
    hipLaunchKernelGGL(mj_k_assign, dim3(P->n_blocks), dim3(64), 0, s, rp);
    // the row counts go to the host BEFORE the snapshot is queued (round 5): the host's read of them (mj_rows_count, one per cycle) and
    // its launch of the encoder then run under the snapshot kernel's 0.1 ms instead of after it
    HIP_OK(hipMemcpyAsync(P->n_rows_host.get(), P->n_rows_dev.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (!P->ev_rows && P->ev_rows.create_no_timing()) return -1;
    HIP_OK(hipEventRecord(P->ev_rows.get(), s));
    SnapParams snp = {P->blocks.get(), P->snap.get(), g_tables.gather, {0}};
    for (int c = 0; c <= SNAP_NCH; c++) snp.chunk_first[c] = g_tables.gather_chunk[c];
    hipLaunchKernelGGL(mj_k_snapshot, dim3(P->n_blocks), dim3(256), 0, s, snp);
    if (!P->ev_snap && P->ev_snap.create_no_timing()) return -1;
    HIP_OK(hipEventRecord(P->ev_snap.get(), s));
    P->step_stream = s;
    HIP_OK(hipGetLastError());
    P->cycles += 1;
    P->rows_valid = false;
    return 0;
}

// ---------------------------------------------------------------- log replay (dataset/gameplay.rs)
int mj_replay_load(MjPool* P, const uint64_t* script, const uint32_t* off, const uint8_t* tracked, int n_logs,
                   int always_include_kan_select, const uint64_t* nonces, const uint64_t* keys) {
    if (!P) return fail("null pool");
    if (n_logs != P->n_tables) return fail("mj_replay_load: one log per table (create the pool with n_tables = n_logs)");
    const size_t n_words = off[n_logs];
    ReplayBufs R;
    if (R.script.alloc(n_words + 1) || R.off.alloc((size_t)n_logs + 1) || R.cursor.alloc(n_logs) || R.ev_index.alloc(n_logs) ||
        R.kyoku.alloc(n_logs) || R.tracked.alloc(n_logs) || R.label.alloc((size_t)n_logs * 4) || R.kan_label.alloc((size_t)n_logs * 4))
        return -1;
    HIP_OK(hipMemcpy(R.script.get(), script, n_words * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(R.off.get(), off, (size_t)(n_logs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(R.tracked.get(), tracked, (size_t)n_logs, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(R.cursor.get(), 0, (size_t)n_logs * sizeof(uint32_t)));
    HIP_OK(hipMemset(R.ev_index.get(), 0, (size_t)n_logs * sizeof(uint32_t)));
    HIP_OK(hipMemset(R.kyoku.get(), 0, (size_t)n_logs));
    R.always_kan = always_include_kan_select;
    std::vector<TableBlock> host = fresh_blocks(P, nonces, keys);  // fresh tables (all seats agent 0)
    HIP_OK(hipMemcpy(P->blocks.get(), host.data(), host.size() * sizeof(TableBlock), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(P->counters.get(), 0, 8 * sizeof(unsigned long long)));
    P->rp = std::move(R);  // (buffers of an earlier load go with R)
    P->rp_active = true;
    P->cycles = 0;
    P->rows_valid = false;
    return 0;
}
int mj_replay_step(MjPool* P, void* stream) {
    if (!P || !P->rp.script) return fail("mj_replay_load first");
    ReplayParams rp;
    rp.blocks = P->blocks.get();
    rp.n_tables = P->n_tables;
    rp.script = P->rp.script.get();
    rp.script_off = P->rp.off.get();
    rp.cursor = P->rp.cursor.get();
    rp.ev_index = P->rp.ev_index.get();
    rp.kyoku_idx = P->rp.kyoku.get();
    rp.tracked = P->rp.tracked.get();
    rp.always_include_kan_select = P->rp.always_kan;
    rp.deal_algo = P->deal_algo;
    rp.block_rows = P->block_rows.get();
    rp.label = P->rp.label.get();
    rp.kan_label = P->rp.kan_label.get();
    rp.counters = P->counters.get();
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mj_k_replay, dim3(P->n_blocks), dim3(64), 0, s, rp);
    return launch_rows(P, s);
}
int mj_replay_meta(MjPool* P, int32_t* meta_dev, void* stream) {
    if (!P || !P->rp.script) return fail("mj_replay_load first");
    if (!P->rows_valid) return fail("mj_rows_count must be called after mj_replay_step");
    const int n = P->last_rows[0];
    if (n == 0) return 0;
    ReplayMetaParams mp = {P->blocks.get(), P->rows[0].get(), n, P->rp.label.get(), P->rp.kan_label.get(), P->rp.kyoku.get(),
                           P->rp.ev_index.get(), meta_dev};
    hipLaunchKernelGGL(mj_k_replay_meta, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mp);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- single-table access (libriichi.state.PlayerState)
int mj_table_apply_event(MjPool* P, int table, const uint64_t* words, int n_words, void* stream) {
    if (!P || table < 0 || table >= P->n_tables) return fail("bad table");
    if (n_words < 1 || n_words > 16) return fail("bad event");
    hipStream_t s = (hipStream_t)stream;
    DevBuf<uint64_t> dev;
    if (dev.alloc(16)) return -1;
    HIP_OK(hipMemcpyAsync(dev.get(), words, (size_t)n_words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(mj_k_apply_event, dim3(1), dim3(1), 0, s, P->blocks.get(), table, dev.get());
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipGetLastError());
    return 0;
}
int mj_table_mark_row(MjPool* P, int table, int seat, int at_kan_select, void* stream) {
    if (!P || table < 0 || table >= P->n_tables || seat < 0 || seat > 3) return fail("bad table / seat");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mj_k_mark_row, dim3(P->n_blocks), dim3(64), 0, s, P->blocks.get(), P->n_tables, table, seat,
                       at_kan_select, P->block_rows.get());
    return launch_rows(P, s);
}
int mj_table_query(MjPool* P, int table, int seat, int what, const int32_t* args8, int32_t* out8, void* stream) {
    if (!P || table < 0 || table >= P->n_tables || seat < 0 || seat > 3) return fail("bad table / seat");
    hipStream_t s = (hipStream_t)stream;
    DevBuf<int32_t> buf;
    if (buf.alloc(16)) return -1;
    int32_t* dev = buf.get();
    HIP_OK(hipMemsetAsync(dev, 0, 16 * sizeof(int32_t), s));
    if (args8) HIP_OK(hipMemcpyAsync(dev, args8, 8 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(mj_k_query, dim3(1), dim3(1), 0, s, P->blocks.get(), table, seat, what, dev, dev + 8);
    HIP_OK(hipMemcpyAsync(out8, dev + 8, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipGetLastError());
    return 0;
}

int mj_rows_count(MjPool* P, int32_t out[2], void* stream) {
    if (!P) return fail("null pool");
    if (P->ev_rows) HIP_OK(hipEventSynchronize(P->ev_rows.get()));  // (the counts' copy; the snapshot queued behind it may still be running)
    else HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    out[0] = P->n_rows_host.get()[0];
    out[1] = P->n_rows_host.get()[1];
    // a batch that does not fit rows[] stays invalid (rows_valid false, last_rows never above max_rows): mj_encode, mj_encode_oracle
    // and mj_replay_meta refuse it with their "mj_rows_count must be called" error instead of walking rows[] past its allocation
    if (out[0] > P->max_rows || out[1] > P->max_rows) return fail("row capacity exceeded");
    P->last_rows[0] = out[0];
    P->last_rows[1] = out[1];
    P->rows_valid = true;
    return 0;
}
const uint32_t* mj_rows_dev(MjPool* P, int agent) { return P ? P->rows[agent & 1].get() : nullptr; }

// What an encode launch reads: the records and the descriptors that index them.  mj_encode / mj_encode_oracle pass the pool's own
// snapshot and row list, a sample store its record array and the descriptors of the requested samples (mj_samples_encode).
struct EncSrc {
    const TableOne* snap;
    const uint32_t* rows;
};
static EncSrc pool_src(const MjPool* P, int agent) { return {P->snap.get(), P->rows[agent & 1].get()}; }

static SpParams sp_params(const EncSrc& src, const SpResources& R, float* obs, int n) {
    SpParams kp{};
    kp.snap = src.snap;
    kp.rows = src.rows;
    kp.n_rows = n;
    kp.tables = g_tables.dev;
    kp.obs = obs;
    kp.work = R.work.get();
    kp.queue = R.queue.get();
    kp.order = R.order.get();
    kp.err = R.err.get();
    return kp;
}

// The SP kernels' resources, sized at the pool's first obs-v4 encode (mj_pool_set_sp_schedule may change the mode until then).
// All or nothing: they are built in a local and moved into the pool last, so after a failure the next v4 encode tries again.
static int sp_setup(MjPool* P, const EncSrc& src, float* obs, hipStream_t s) {
    SpResources R;
    const PoolKnobs& K = P->knobs;
    if (R.err.alloc(SP_ERR_WORDS)) return -1;
    HIP_OK(hipMemset(R.err.get(), 0, SP_ERR_WORDS * sizeof(unsigned long long)));
    if (R.order.alloc(P->max_rows) || R.cls.alloc(P->max_rows)) return -1;
    // persistent workgroups: SP_WGS per CU, one decision row each at a time; never more than the rows of a launch (small pools: small work area)
    R.grid = std::min(256 * SP_WGS, P->max_rows);
    if (K.sp_grid) R.grid = std::max(1, std::min(R.grid, *K.sp_grid));
    const bool env = !P->sp_sched_set;  // the environment's schedule applies (to the pool: with the resources, below)
    const int wide_mode = env && K.sp_wide ? *K.sp_wide : P->sp_wide_mode;
    const int wide_max_rows = env && K.sp_wide_max_rows ? *K.sp_wide_max_rows : P->sp_wide_max_rows;
    R.spare = wide_mode == 0 ? 0 : std::min(SP_PROMO_CAP, std::max(8, P->n_tables / 4) & ~1);
    if (wide_mode < 0 && P->n_tables > wide_max_rows) R.spare = 0;  // (a launch has about as many rows as the pool has tables)
    R.wide_areas = R.spare ? std::min(256, std::max(2, P->n_tables / 16)) : 0;  // (a 64-table test pool does not need 2 GB of work areas)
    const int areas = R.grid + R.spare + R.wide_areas;
    if (R.work.alloc(areas)) return -1;
    for (int g = 0; g < areas; g++) {
        SpWork& W = R.work.get()[g];
        HIP_OK(hipMemsetAsync(W.tag, 0, sizeof(W.tag), s));  // empty hash sets ...
        HIP_OK(hipMemsetAsync(&W.epoch, 0, sizeof(W.epoch) + sizeof(W.pad_), s));  // ... at epoch 0
        HIP_OK(hipMemsetAsync(&W.node[SP_ZERO_SLOT], 0, sizeof(SpNode), s));  // the child of a dead tenpai level's draw entries: zeros, never written
    }
    if (R.queue.alloc(SP_Q_WORDS)) return -1;
    if (R.spare) {
        if (R.stream2.create_non_blocking() || R.ev_fork.create_no_timing() || R.ev_join.create_no_timing() || R.gaveup_host.alloc(1)) return -1;
        *R.gaveup_host.get() = 0ull;
        // One empty launch of the pair now: the HIP runtime sizes a queue's scratch at the first launch that needs it, and a caller
        // whose allocator has taken the whole HBM by then (torch's caching allocator under a growing batch) turns that into
        // HSA_STATUS_ERROR_OUT_OF_RESOURCES in the middle of a run -- at pool set-up it is an ordinary, early failure.
        HIP_OK(hipMemsetAsync(R.queue.get(), 0, SP_Q_WORDS * sizeof(int), s));
        HIP_OK(hipStreamSynchronize(s));
        SpParams w = sp_params(src, R, obs, 0);
        w.sweep = 1;
        hipLaunchKernelGGL(mj_k_sp_wide, dim3(1), dim3(SP_WIDE_THREADS), 0, s, w);
        hipLaunchKernelGGL(mj_k_sp_promo, dim3(1), dim3(SP_THREADS), 0, R.stream2.get(), w);
        HIP_OK(hipStreamSynchronize(R.stream2.get()));
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipGetLastError());
    }
    P->sp = std::move(R);
    P->sp_wide_mode = wide_mode;
    P->sp_wide_max_rows = wide_max_rows;
    if (env && K.sp_wide_grid) P->sp_wide_grid = std::max(1, *K.sp_wide_grid);
    if (env && K.sp_promo_min1) P->sp_promo_min[1] = std::max(1, *K.sp_promo_min1);
    if (env && K.sp_promo_min2) P->sp_promo_min[2] = std::max(1, *K.sp_promo_min2);
    return 0;
}

// One SP launch over the n rows just encoded: the row order, then mj_k_sp alone or the small-pool schedule
static int sp_launch(MjPool* P, const EncSrc& src, float* obs, int n, hipStream_t s) {
    SpResources& R = P->sp;
    HIP_OK(hipMemsetAsync(R.queue.get(), 0, SP_Q_WORDS * sizeof(int), s));
    SpParams kp = sp_params(src, R, obs, n);
    kp.prof = P->knobs.sp_prof ? R.err.get() : nullptr;
    const int grid = std::min(n, R.grid);
    // The schedule needs mj_k_sp_wide and mj_k_sp_promo side by side.  Where they do not overlap -- more streams in the process than the
    // runtime has hardware queues, so that the promo kernel queues up BEHIND the spinning wide kernel -- the wide workgroups give up
    // after SP_WIDE_TIMEOUT, the sweep launch still produces the same obs, and the give-ups (copied to pinned memory behind every
    // sweep) switch the schedule off for this pool: one slow launch, then mj_k_sp alone as in round 5.
    if (P->sp_wide_mode < 0 && R.gaveup_host && *R.gaveup_host.get() && !P->sp_wide_off) {  // (auto mode only: mode 1 = every launch, as asked)
        P->sp_wide_off = true;
        fprintf(stderr, "[mortal_amd] small-pool SP schedule switched off for this pool: mj_k_sp_wide and mj_k_sp_promo did not run side by side "
                        "(%llu wide workgroups gave up waiting; more concurrent streams than hardware queues?)\n", *R.gaveup_host.get());
    }
    const bool hybrid = R.spare > 0 && !P->sp_wide_off && (P->sp_wide_mode > 0 || (P->sp_wide_mode < 0 && n <= P->sp_wide_max_rows));
    kp.promo_cap = hybrid ? R.spare : 0;
    // Defaults measured on MI355X: up to ~12 k rows 64 wide workgroups (a quarter of the CUs),
    // rows parked at >= 1,200 level-1 states (or >= 400 level-2 states, before that level is expanded); up to ~20 k rows 32 wide
    // workgroups and 1,600 level-1 states; beyond that a launch keeps all CUs for mj_k_sp (sp_wide_max_rows).  The root level is never
    // parked (nothing is known yet), level 0 is not expanded.
    kp.promo_min[0] = kp.promo_min[3] = 1 << 30;
    kp.promo_min[1] = P->sp_promo_min[1] > 0 ? P->sp_promo_min[1] : n <= 12000 ? 1200 : 1600;
    kp.promo_min[2] = P->sp_promo_min[2] > 0 ? P->sp_promo_min[2] : n <= 12000 ? 400 : 1 << 30;
    kp.n_narrow = grid;
    // queue order: rows counting-sorted by cost class, heaviest first (inside the timed mj_k_sp region)
    hipLaunchKernelGGL(mj_k_order_classify, dim3((n + 255) / 256), dim3(256), 0, s, src.snap, kp.rows, n, R.cls.get(), R.queue.get() + 1);
    hipLaunchKernelGGL(mj_k_order_scatter, dim3((n + 255) / 256), dim3(256), 0, s, R.cls.get(), n, R.queue.get() + 1, R.queue.get() + 9,
                       R.order.get());
    if (!hybrid) {
        hipLaunchKernelGGL(mj_k_sp, dim3(grid), dim3(SP_THREADS), 0, s, kp);
    } else {
        // mj_k_sp_wide FIRST and on the caller's stream (its few workgroups take a whole CU each and must be resident before the 1,024
        // workgroups of mj_k_sp fill the chip), mj_k_sp on the second stream behind the row order, then the sweep behind both.
        // The emulator runs a launch to completion: there (and with MJ_SP_WIDE_SERIAL=1) the sweep alone takes the parked rows.
        P->sp_hybrid_launches++;
        const int wgrid = std::min(R.wide_areas, P->sp_wide_grid > 0 ? P->sp_wide_grid : n <= 12000 ? 64 : 32);
        if (P->knobs.sp_wide_serial) {
            if (P->knobs.sp_wide_all_rows) {  // (tests) the wide kernel alone first: with no producer to wait for it takes EVERY row of the queue itself
                SpParams spw = kp;
                spw.n_narrow = 0;
                spw.work = kp.work + grid;  // (its own areas: work + n_narrow + promo_cap + block, as in the concurrent launch)
                hipLaunchKernelGGL(mj_k_sp_wide, dim3(wgrid), dim3(SP_WIDE_THREADS), 0, s, spw);
            }
            hipLaunchKernelGGL(mj_k_sp_promo, dim3(grid), dim3(SP_THREADS), 0, s, kp);
        } else {
            HIP_OK(hipEventRecord(R.ev_fork.get(), s));
            hipLaunchKernelGGL(mj_k_sp_wide, dim3(wgrid), dim3(SP_WIDE_THREADS), 0, s, kp);
            HIP_OK(hipStreamWaitEvent(R.stream2.get(), R.ev_fork.get(), 0));
            hipLaunchKernelGGL(mj_k_sp_promo, dim3(grid), dim3(SP_THREADS), 0, R.stream2.get(), kp);
            HIP_OK(hipEventRecord(R.ev_join.get(), R.stream2.get()));
            HIP_OK(hipStreamWaitEvent(s, R.ev_join.get(), 0));
        }
        kp.sweep = 1;
        hipLaunchKernelGGL(mj_k_sp_wide, dim3(wgrid), dim3(SP_WIDE_THREADS), 0, s, kp);
        HIP_OK(hipMemcpyAsync(R.gaveup_host.get(), R.err.get() + SP_ERR_WIDE_GAVEUP, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    return 0;
}

// The launches of one encode over rows [0, n) of `src`: the encoder of C's obs version for `agent`, then for obs v4 the SP block.  C owns
// what they need beside the records: version, the op-list flag, the SP resources (set up at the first v4 call), knobs and timers.
static int encode_launch(MjPool* C, int agent, const EncSrc& src, int n, float* obs, uint8_t* masks, hipStream_t s) {
    EncParams ep;
    ep.blocks = C->blocks.get();
    ep.rows = src.rows;
    ep.n_rows = n;
    ep.tables = g_tables.dev;
    ep.obs = obs;
    ep.masks = masks;
    ep.version = C->version[agent & 1];
    ep.C = mj_obs_rows(ep.version);
    ep.snap = src.snap;
    ep.decay_lut = g_tables.decay;
    ep.rbf_score = g_tables.rbf_score;
    ep.rbf_6 = g_tables.rbf_6;
    ep.rbf_12 = g_tables.rbf_12;
    ep.rbf_23 = g_tables.rbf_23;
    ep.err_flag = C->enc_flag.get();
    size_t lds = enc_lds_bytes(ep.version);
    if (C->timing && C->enc_timer.begin(s)) return -1;
    switch (ep.version) {
        case 1: hipLaunchKernelGGL(mj_k_encode<1>, dim3(n), dim3(ENC_THREADS), lds, s, ep); break;
        case 2: hipLaunchKernelGGL(mj_k_encode<2>, dim3(n), dim3(ENC_THREADS), lds, s, ep); break;
        case 3: hipLaunchKernelGGL(mj_k_encode<3>, dim3(n), dim3(ENC_THREADS), lds, s, ep); break;
        default: hipLaunchKernelGGL(mj_k_encode<4>, dim3(n), dim3(ENC_THREADS), lds, s, ep); break;
    }
    if (C->timing && C->enc_timer.end(s)) return -1;
    HIP_OK(hipGetLastError());
    if (ep.version != 4) return 0;
    // SP block, rows 889..1011: one decision row per persistent workgroup (mj_sp.hip: mj_k_sp; the per-phase pipeline of round 4 that
    // lost to it: DESIGN.md section 6)
    if (!C->sp.work && sp_setup(C, src, obs, s)) return -1;
    if (C->timing && C->sp_timer.begin(s)) return -1;
    if (sp_launch(C, src, obs, n, s)) return -1;
    if (C->timing && C->sp_timer.end(s)) return -1;
    HIP_OK(hipGetLastError());
    return 0;
}

int mj_encode(MjPool* P, int agent, float* obs, uint8_t* masks, void* stream) {
    if (!P) return fail("null pool");
    if (!P->rows_valid) return fail("mj_rows_count must be called after mj_step and before mj_encode");
    int n = P->last_rows[agent & 1];
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (wait_snapshot(P, s)) return -1;
    return encode_launch(P, agent, pool_src(P, agent), n, obs, masks, s);
}

int mj_oracle_obs_rows(int version) {  // consts.rs:32-38
    if (version == 1) return 211;
    if (version >= 2 && version <= 4) return 217;
    return -1;
}

// The invisible obs of rows [0, n) of `src`, at `version`; all_yama: every undrawn yama tile is listed (replayed games)
static int encode_oracle_launch(int version, const EncSrc& src, int n, float* out, int all_yama, hipStream_t s) {
    OracleEncParams ep;
    ep.rows = src.rows;
    ep.n_rows = n;
    ep.version = version;
    ep.snap = src.snap;
    ep.out = out;
    ep.all_yama = all_yama;
    size_t lds = enc_oracle_lds_bytes(ep.version);
    if (ep.version == 1) hipLaunchKernelGGL(mj_k_encode_oracle<true>, dim3(n), dim3(ENC_THREADS), lds, s, ep);
    else hipLaunchKernelGGL(mj_k_encode_oracle<false>, dim3(n), dim3(ENC_THREADS), lds, s, ep);
    HIP_OK(hipGetLastError());
    return 0;
}

int mj_encode_oracle(MjPool* P, int agent, float* out, void* stream) {
    if (!P) return fail("null pool");
    if (!P->rows_valid) return fail("mj_rows_count must be called after mj_step and before mj_encode_oracle");
    int n = P->last_rows[agent & 1];
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (wait_snapshot(P, s)) return -1;
    return encode_oracle_launch(P->version[agent & 1], pool_src(P, agent), n, out, P->rp_active ? 1 : 0, s);
}

int mj_encode_timing(MjPool* P, int enable, double* total_ms, int64_t* launches) {
    if (!P) return fail("null pool");
    P->enc_timer.collect(total_ms, launches);
    P->timing = enable != 0;
    return 0;
}

int mj_sp_timing(MjPool* P, double* total_ms, int64_t* launches) {
    if (!P) return fail("null pool");
    P->sp_timer.collect(total_ms, launches);
    return 0;
}

int mj_random_policy(MjPool* P, int agent, const uint8_t* masks, uint64_t seed, uint64_t cycle, int32_t* actions,
                     void* stream) {
    if (!P) return fail("null pool");
    if (!P->rows_valid) return fail("mj_rows_count must be called first");
    int n = P->last_rows[agent & 1];
    if (n == 0) return 0;
    hipLaunchKernelGGL(mj_k_random_policy, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P->blocks.get(),
                       P->rows[agent & 1].get(), masks, n, seed, cycle, actions);
    HIP_OK(hipGetLastError());
    return 0;
}

int mj_greedy_policy(MjPool* P, int agent, const uint8_t* masks, const float* obs, uint64_t seed, uint64_t cycle,
                     int32_t* actions, void* stream) {
    if (!P) return fail("null pool");
    if (!P->rows_valid) return fail("mj_rows_count must be called first");
    int n = P->last_rows[agent & 1];
    if (n == 0) return 0;
    const int v = P->version[agent & 1];
    const int d0 = v == 1 ? 923 : v == 2 ? 927 : v == 3 ? 919 : 874;  // first row of the discard block (obs_repr.rs:431-476)
    hipLaunchKernelGGL(mj_k_greedy_policy, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P->rows[agent & 1].get(), masks,
                       obs, mj_obs_rows(v), d0, n, seed, cycle, actions);
    HIP_OK(hipGetLastError());
    return 0;
}

int mj_counters(MjPool* P, uint64_t out[8], void* stream) {
#ifdef MJ_STEP_PROF
    if (getenv("MJ_STEP_PROF")) {
        unsigned long long sp_[32];
        hipDeviceSynchronize();
        if (hipMemcpyFromSymbol(sp_, HIP_SYMBOL(g_step_prof), sizeof sp_) == hipSuccess) {
            fprintf(stderr, "[step prof] waves %llu kernel %llu commit %llu poll %llu (start_kyoku %llu board_step %llu [n %llu] any_can_act %llu; kyoku ends %llu) classify %llu | board_step by event:",
                    sp_[8], sp_[0], sp_[1], sp_[2], sp_[3], sp_[4], sp_[9], sp_[5], sp_[10], sp_[7]);
            for (int k = 11; k < 32; k++) fprintf(stderr, " %llu", sp_[k]);
            fprintf(stderr, "\n");
        }
    }
#endif
    if (!P) return fail("null pool");
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long tmp[8];
    HIP_OK(hipMemcpy(tmp, P->counters.get(), sizeof tmp, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; i++) out[i] = tmp[i];
    out[5] = P->cycles;
    int f = 0;
    HIP_OK(hipMemcpy(&f, P->enc_flag.get(), sizeof f, hipMemcpyDeviceToHost));
    out[6] = (unsigned long long)f;  // (the SP block's overflows are added below)
    if (P->sp.err) {
        unsigned long long e2[SP_ERR_WORDS];
        HIP_OK(hipMemcpy(e2, P->sp.err.get(), sizeof e2, hipMemcpyDeviceToHost));
        out[6] += e2[SP_ERR_OVERFLOW];
        out[7] = e2[SP_ERR_ROWS];
        const unsigned long long* pass = e2 + SP_ERR_PASS;  // (seven words: SpCtx::pt[0..6])
        if (P->knobs.sp_prof)
            fprintf(stderr, "[sp prof] rows %llu setup %llu expand %llu evalL0 %llu evalL>0 %llu encode %llu states %llu (wall_clock64 ticks, 100 MHz) | "
                    "expand passes: probes %llu lists+V %llu td-probes %llu layout %llu inserts %llu; items %llu expanded %llu edges %llu l0-entries %llu; level-0 probe %llu scoring %llu; workgroup lifetimes: sum %llu max %llu queue pops %llu hash resets %llu; eval wavefront time %llu; shader clock %.0f MHz (s_memtime cycles %llu over the lifetimes); dead-leaf rows %llu\n",
                    e2[SP_ERR_ROWS], e2[SP_ERR_T_SETUP], e2[SP_ERR_T_EXPAND], e2[SP_ERR_T_EVAL0], e2[SP_ERR_T_EVAL], e2[SP_ERR_T_WRITE], e2[SP_ERR_STATES],
                    pass[0], pass[1], pass[2], pass[3], pass[4], pass[5], pass[6], e2[SP_ERR_EDGES], e2[SP_ERR_L0_ITEMS],
                    e2[SP_ERR_T_L0_PROBE], e2[SP_ERR_T_L0_SCORE], e2[SP_ERR_WG_LIFE], e2[SP_ERR_WG_LIFE_MAX], e2[SP_ERR_T_POP], e2[SP_ERR_T_RESET],
                    e2[SP_ERR_T_EVAL_WAVE], e2[SP_ERR_WG_LIFE] ? 100.0 * (double)e2[SP_ERR_WG_CLOCK] / (double)e2[SP_ERR_WG_LIFE] : 0.0,
                    e2[SP_ERR_WG_CLOCK], e2[SP_ERR_DEAD_LEAF]);
    }
    return 0;
}

#ifdef MJ_EMU
// emulator builds only (not part of the C-ABI): states placed in mj_k_sp's LDS set / in the HBM table since the library was loaded
void mj_emu_sp_placed(uint64_t out[2]) { out[0] = g_sp_emu_placed[0]; out[1] = g_sp_emu_placed[1]; }
// claims lost since then: LDS set to the same id / to another id, HBM table to the same id / to another id (mj_sp.hip: g_sp_emu_lost)
void mj_emu_sp_lost_claims(uint64_t out[4]) {
    for (int k = 0; k < 2; k++) out[k] = g_sp_emu_lost[2 + k], out[2 + k] = g_sp_emu_lost[k] - g_sp_emu_lost[2 + k];
}
// paths of the expansion's insert pass taken since then (mj_sp.hip: g_sp_emu_paths)
void mj_emu_sp_insert_paths(uint64_t out[6]) {
    for (int k = 0; k < 6; k++) out[k] = g_sp_emu_paths[k];
}
#ifdef MJ_EMU_REGISTRY
// the emulated runtime's registry (tests/host/emu/hip/hip_runtime.h): live buffers (device and pinned) / events / streams, frees and
// destroys of something not live, allocations and stream synchronises made since the library was loaded
void mj_emu_alloc_stats(uint64_t out[6]) {
    const emu::Registry& r = emu::R();
    out[0] = r.buffers.size(), out[1] = r.events.size(), out[2] = r.streams.size(), out[3] = r.bad_frees, out[4] = r.allocs, out[5] = r.syncs;
}
// the nth allocation / the nth stream synchronise from now on fails, once (<= 0: none does)
void mj_emu_fail_nth(int alloc, int sync) { emu::R().fail_alloc_in = alloc, emu::R().fail_sync_in = sync; }
#endif
#endif

int mj_sp_phase_ticks(MjPool* P, uint64_t out[9], void* stream) {
    if (!P) return fail("null pool");
    for (int i = 0; i < 9; i++) out[i] = 0;
    if (!P->sp.err) return 0;  // no obs-v4 encode has run yet
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long e2[SP_ERR_WORDS];
    HIP_OK(hipMemcpy(e2, P->sp.err.get(), sizeof e2, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; i++) out[i] = e2[i];  // SP_ERR_OVERFLOW .. SP_ERR_STATES
    out[8] = e2[SP_ERR_DEAD_LEAF];
    return 0;
}

int mj_pool_set_sp_schedule(MjPool* P, int mode, int max_rows, int wide_grid, int min_level1, int min_level2) {
    if (!P) return fail("null pool");
    if (P->sp.work && mode != 0 && mode >= -1 && P->sp.spare == 0) return fail("mj_pool_set_sp_schedule: the work areas are allocated (call it before the first obs-v4 mj_encode)");
    if (mode >= -1) P->sp_wide_mode = mode > 0 ? 1 : mode;
    if (max_rows > 0) P->sp_wide_max_rows = max_rows;
    if (wide_grid > 0) P->sp_wide_grid = std::min(wide_grid, 256);
    if (min_level1 > 0) P->sp_promo_min[1] = min_level1;
    if (min_level2 > 0) P->sp_promo_min[2] = min_level2;
    P->sp_sched_set = true;
    return 0;
}

int mj_sp_schedule_stats(MjPool* P, uint64_t out[4], void* stream) {
    if (!P) return fail("null pool");
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (!P->sp.err) return 0;
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long e2[SP_ERR_WORDS];
    HIP_OK(hipMemcpy(e2, P->sp.err.get(), sizeof e2, hipMemcpyDeviceToHost));
    out[0] = P->sp_hybrid_launches;
    out[1] = e2[SP_ERR_PROMOTED];
    out[2] = e2[SP_ERR_SWEPT];
    out[3] = e2[SP_ERR_WIDE_GAVEUP];
    return 0;
}

int mj_results(MjPool* P, int32_t* scores, uint8_t* done, void* stream) {
    if (!P) return fail("null pool");
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    HIP_OK(hipMemcpy(scores, P->final_scores.get(), (size_t)P->n_games_total * 4 * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(done, P->final_done.get(), (size_t)P->n_games_total, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- packed event logs as a source (mj_log.h LogSrc)
namespace {
// grid of the wavefront-per-log kernels; MJ_LOG_GRID caps it (tests: few workgroups, many logs each)
int log_grid(size_t n_logs) {
    int grid = (int)std::min<size_t>((n_logs + LOG_WAVES - 1) / LOG_WAVES, LOG_GRID_MAX);
    if (const char* v = getenv("MJ_LOG_GRID")) grid = std::min(grid, atoi(v));
    return std::max(grid, 1);
}
// concatenated host logs on the device, with their owners; n_logs == 0: nothing is uploaded and src.n_logs stays 0
struct HostLogs {
    DevBuf<uint64_t> words;
    DevBuf<uint32_t> off;
    LogSrc src{};
};
int upload_logs(const std::string& who, const uint64_t* words_host, const uint32_t* off_host, int n_logs, hipStream_t s, HostLogs& L) {
    if (n_logs <= 0) return n_logs < 0 ? fail(who + ": negative n_logs") : 0;
    if (!off_host) return fail(who + ": null offsets");
    for (int i = 0; i < n_logs; i++)  // the kernels trust the offsets: a log lies inside [0, off[n_logs])
        if (off_host[i] > off_host[i + 1]) return fail(who + ": offsets of log " + std::to_string(i) + " decrease");
    const size_t n_words = off_host[n_logs];
    if (n_words && !words_host) return fail(who + ": null words");
    if (stat_upload(L.words, words_host, n_words, s) || stat_upload(L.off, off_host, (size_t)n_logs + 1, s)) return -1;
    L.src.words = L.words.get();
    L.src.off = L.off.get();
    L.src.n_logs = n_logs;
    return 0;
}
// tables [table0, table0 + n) of a pool's log as a source, read behind its last step.  `log_of`: how the message names the log;
// `instead`: what a pool in refill mode is pointed to
int pool_log_src(const std::string& who, MjPool* P, int table0, int n, hipStream_t s, LogSrc& S,
                 const char* instead, const char* log_of = "the event log") {
    if (!P->log) return fail(who + ": " + log_of + " is not enabled (mj_pool_enable_log)");
    if (P->refill_stride)
        return fail(who + ": not available in refill mode (a restarted table's log has been rewound; " + instead + " collected games)");
    if (table0 < 0 || table0 > P->n_tables - n) return fail(who + ": table range out of bounds");
    if (wait_snapshot(P, s)) return -1;  // behind the last step, whatever its stream
    S = LogSrc{};
    S.words = P->log.get();
    S.len = P->log_len.get();
    S.stride = P->log_cap;
    S.blocks = P->blocks.get();
    S.table0 = table0;
    S.n_logs = n;
    return 0;
}

// ---------------------------------------------------------------- Stat over event logs (stat.rs:263-441; mj_stat.hip)
int stat_args(int64_t* totals_out, int64_t* counts_out) {
    if (!totals_out || !counts_out) return fail("null totals / counts buffer");
    memset(totals_out, 0, 2 * MJ_STAT_FIELDS * sizeof(int64_t));
    memset(counts_out, 0, 3 * sizeof(int64_t));
    return 0;
}
// launches mj_k_log_stat with K's inputs, copies the outputs to the host and waits for them
int stat_run(StatParams K, const uint8_t* seats_host, int64_t* totals_out, int64_t* per_seat_out, int64_t counts_out[3],
             hipStream_t s) {
    if (!totals_out || !counts_out) return fail("null totals / counts buffer");
    const size_t n = (size_t)K.src.n_logs, n_out = 2 * MJ_STAT_FIELDS + 3;
    DevBuf<uint8_t> b_seats;
    DevBuf<unsigned long long> b_out;
    DevBuf<long long> b_per;
    if (seats_host) {
        if (stat_upload(b_seats, seats_host, n, s)) return -1;
        K.seats = b_seats.get();
    }
    if (b_out.alloc(n_out)) return -1;
    HIP_OK(hipMemsetAsync(b_out.get(), 0, n_out * sizeof(int64_t), s));
    K.totals = b_out.get();
    K.counts = K.totals + 2 * MJ_STAT_FIELDS;
    if (per_seat_out) {
        if (b_per.alloc(n * 4 * MJ_STAT_FIELDS)) return -1;
        K.per_seat = b_per.get();
    }
    hipLaunchKernelGGL(mj_k_log_stat, dim3(log_grid(n)), dim3(LOG_THREADS), 0, s, K);
    HIP_OK(hipGetLastError());
    int64_t out[2 * MJ_STAT_FIELDS + 3];
    HIP_OK(hipMemcpyAsync(out, b_out.get(), sizeof out, hipMemcpyDeviceToHost, s));
    if (per_seat_out)
        HIP_OK(hipMemcpyAsync(per_seat_out, b_per.get(), n * 4 * MJ_STAT_FIELDS * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    memcpy(totals_out, out, 2 * MJ_STAT_FIELDS * sizeof(int64_t));
    memcpy(counts_out, out + 2 * MJ_STAT_FIELDS, 3 * sizeof(int64_t));
    return 0;
}
}  // namespace

int mj_stat_logs(const uint64_t* words_host, const uint32_t* off_host, int n_logs, const uint8_t* seats_host,
                 const uint8_t* groups_host, int64_t* totals_out, int64_t* per_seat_out, int64_t counts_out[3], void* stream) {
    if (stat_args(totals_out, counts_out)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HostLogs L;
    DevBuf<uint8_t> b_groups;
    if (upload_logs("mj_stat_logs", words_host, off_host, n_logs, s, L)) return -1;
    if (!L.src.n_logs) return 0;
    StatParams K{};
    K.src = L.src;
    if (groups_host) {
        if (stat_upload(b_groups, groups_host, (size_t)n_logs, s)) return -1;
        K.groups = b_groups.get();
    }
    return stat_run(K, seats_host, totals_out, per_seat_out, counts_out, s);
}

int mj_pool_stat(MjPool* P, const uint8_t* seats_host, int64_t* totals_out, int64_t* per_seat_out, int64_t counts_out[3],
                 void* stream) {
    if (!P) return fail("null pool");
    StatParams K{};
    if (pool_log_src("mj_pool_stat", P, 0, P->n_tables, (hipStream_t)stream, K.src, "mj_harvest_stat reads")) return -1;
    return stat_run(K, seats_host, totals_out, per_seat_out, counts_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------- samples and Grp from packed logs (mj_gameplay.hip)
namespace {
// launches mj_k_log_grp over S, copies the outputs to the host and waits for them
int grp_run(const LogSrc& S, int max_kyoku, int32_t* feat_out, int32_t* n_kyoku_out, int32_t* rank_out, int32_t* final_out,
            int64_t counts_out[3], hipStream_t s) {
    const size_t n = (size_t)S.n_logs, n_feat = n * (size_t)max_kyoku * 7;
    DevBuf<int32_t> b_feat, b_small;  // b_small: n_kyoku [n], rank [n][4], final [n][4]
    DevBuf<unsigned long long> b_counts;
    if (b_feat.alloc(n_feat) || b_small.alloc(n * 9) || b_counts.alloc(3)) return -1;
    HIP_OK(hipMemsetAsync(b_feat.get(), 0, n_feat * sizeof(int32_t), s));
    HIP_OK(hipMemsetAsync(b_counts.get(), 0, 3 * sizeof(unsigned long long), s));
    const GrpParams K = {S, max_kyoku, b_feat.get(), b_small.get(), b_small.get() + n, b_small.get() + n * 5, b_counts.get()};
    hipLaunchKernelGGL(mj_k_log_grp, dim3(log_grid(n)), dim3(LOG_THREADS), 0, s, K);
    HIP_OK(hipGetLastError());
    int64_t counts[3];
    HIP_OK(hipMemcpyAsync(feat_out, K.feat, n_feat * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(n_kyoku_out, K.n_kyoku, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(rank_out, K.rank, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(final_out, K.final_, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(counts, K.counts, sizeof counts, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    memcpy(counts_out, counts, sizeof counts);
    return 0;
}
int grp_args(const char* who, int n, int max_kyoku, const void* feat, const void* n_kyoku, const void* rank, const void* final_,
             int64_t* counts_out) {
    if (!counts_out) return fail(std::string(who) + ": null counts buffer");
    memset(counts_out, 0, 3 * sizeof(int64_t));
    if (n < 0) return fail(std::string(who) + ": negative number of logs");
    if (max_kyoku < 1) return fail(std::string(who) + ": max_kyoku must be at least 1");
    if (n && (!feat || !n_kyoku || !rank || !final_)) return fail(std::string(who) + ": null output buffer");
    return 0;
}
}  // namespace

int mj_grp_logs(const uint64_t* words_host, const uint32_t* off_host, int n_logs, int max_kyoku, int32_t* feat_out,
                int32_t* n_kyoku_out, int32_t* rank_out, int32_t* final_out, int64_t counts_out[3], void* stream) {
    if (grp_args("mj_grp_logs", n_logs, max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HostLogs L;
    if (upload_logs("mj_grp_logs", words_host, off_host, n_logs, s, L)) return -1;
    if (!L.src.n_logs) return 0;
    return grp_run(L.src, max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out, s);
}

int mj_pool_grp(MjPool* P, int table0, int n, int max_kyoku, int32_t* feat_out, int32_t* n_kyoku_out, int32_t* rank_out,
                int32_t* final_out, int64_t counts_out[3], void* stream) {
    if (!P) return fail("null pool");
    if (grp_args("mj_pool_grp", n, max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out)) return -1;
    LogSrc S;
    if (pool_log_src("mj_pool_grp", P, table0, n, (hipStream_t)stream, S, "mj_harvest_grp reads")) return -1;
    if (n == 0) return 0;
    return grp_run(S, max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out, (hipStream_t)stream);
}

namespace {
// mj_k_log_len -> mj_k_log_scan -> mj_k_log_pack over S: log i goes to out[off[i] .. off[i + 1]), an empty range for a skipped or
// malformed one.  len [n], off [n + 1]; sums [4], zeroed by the caller: the three counts and the total of words.  `get_out(out)`
// is asked for the output between scan and pack, so that a caller may size it by the total (it waits for sums[3] itself).
int log_pack_run(const LogSrc& S, uint32_t* len, uint32_t* off, unsigned long long* sums, const std::function<int(uint64_t*&)>& get_out,
                 bool augment, int deal_from_seed, hipStream_t s) {
    const int grid = log_grid((size_t)S.n_logs);
    const LogLenParams lp = {S, len, sums};
    hipLaunchKernelGGL(mj_k_log_len, dim3(grid), dim3(LOG_THREADS), 0, s, lp);
    hipLaunchKernelGGL(mj_k_log_scan, dim3(1), dim3(1024), 0, s, len, S.n_logs, off, sums + 3);
    HIP_OK(hipGetLastError());
    uint64_t* out = nullptr;
    if (get_out(out)) return -1;
    const LogPackParams pp = {S, off, out, deal_from_seed};
    if (augment) hipLaunchKernelGGL(mj_k_log_pack<true>, dim3(grid), dim3(LOG_THREADS), 0, s, pp);
    else hipLaunchKernelGGL(mj_k_log_pack<false>, dim3(grid), dim3(LOG_THREADS), 0, s, pp);
    HIP_OK(hipGetLastError());
    return 0;
}
// where the destination's tables take their seeds from (deal_from_seed): the source pool's tables, or plain device arrays
struct SeedSrc {
    const TableBlock* blocks;
    int table0;
    const uint64_t *nonces, *keys;
};
// The load shared by mj_replay_load_pool and mj_replay_load_harvest: the logs of S become dst's replay scripts, on the device.
// Everything is built beside the destination and moved in last: its tables and counters too, so that no failure -- the last
// synchronise included -- can leave it between two scripts.
int replay_load_src(const std::string& who, MjPool* dst, const LogSrc& S, const SeedSrc& seeds, const uint8_t* tracked_host,
                    int always_include_kan_select, int flags, int64_t counts_out[3], hipStream_t s) {
    if (flags & ~(MJ_LOAD_DEAL_FROM_SEED | MJ_LOAD_AUGMENT))
        return fail(who + ": unknown load flags " + std::to_string(flags) + " (MJ_LOAD_DEAL_FROM_SEED | MJ_LOAD_AUGMENT)");
    const int deal_from_seed = flags & MJ_LOAD_DEAL_FROM_SEED;
    const int n = dst->n_tables;
    ReplayBufs R;
    DevBuf<TableBlock> blocks;
    DevBuf<unsigned long long> counters, sums;  // sums: loaded / skipped / malformed, total words
    DevBuf<uint32_t> len;
    if (R.off.alloc((size_t)n + 1) || R.cursor.alloc(n) || R.ev_index.alloc(n) || R.kyoku.alloc(n) || R.tracked.alloc(n) ||
        R.label.alloc((size_t)n * 4) || R.kan_label.alloc((size_t)n * 4) || blocks.alloc(dst->n_blocks) || counters.alloc(8) ||
        sums.alloc(4) || len.alloc(n))
        return -1;
    if (tracked_host) HIP_OK(hipMemcpyAsync(R.tracked.get(), tracked_host, (size_t)n, hipMemcpyHostToDevice, s));
    else HIP_OK(hipMemsetAsync(R.tracked.get(), 0x0F, (size_t)n, s));
    HIP_OK(hipMemsetAsync(R.cursor.get(), 0, (size_t)n * sizeof(uint32_t), s));
    HIP_OK(hipMemsetAsync(R.ev_index.get(), 0, (size_t)n * sizeof(uint32_t), s));
    HIP_OK(hipMemsetAsync(R.kyoku.get(), 0, (size_t)n, s));
    HIP_OK(hipMemsetAsync(blocks.get(), 0, (size_t)dst->n_blocks * sizeof(TableBlock), s));
    HIP_OK(hipMemsetAsync(counters.get(), 0, 8 * sizeof(unsigned long long), s));
    HIP_OK(hipMemsetAsync(sums.get(), 0, 4 * sizeof(unsigned long long), s));
    R.always_kan = always_include_kan_select;
    const SeedSrc sd = deal_from_seed ? seeds : SeedSrc{nullptr, 0, nullptr, nullptr};
    hipLaunchKernelGGL(mj_k_log_fresh, dim3(dst->n_blocks), dim3(64), 0, s, blocks.get(), n, sd.blocks, sd.table0, sd.nonces, sd.keys);
    unsigned long long sums_host[4];
    auto script = [&](uint64_t*& out) {  // allocated once the total is known
        HIP_OK(hipMemcpyAsync(sums_host, sums.get(), sizeof sums_host, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        if (sums_host[3] > 0xFFFFFFFFull)
            return fail(who + ": " + std::to_string(sums_host[3]) + " script words do not fit the 32-bit offsets: load fewer tables per call");
        if (R.script.alloc((size_t)sums_host[3] + 1)) return -1;
        out = R.script.get();
        return 0;
    };
    if (log_pack_run(S, len.get(), R.off.get(), sums.get(), script, (flags & MJ_LOAD_AUGMENT) != 0, deal_from_seed, s)) return -1;
    HIP_OK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) counts_out[k] = (int64_t)sums_host[k];
    dst->blocks = std::move(blocks);  // (what the destination held goes with the locals)
    dst->counters = std::move(counters);
    dst->rp = std::move(R);
    dst->rp_active = true;
    dst->cycles = 0;
    dst->rows_valid = false;
    return 0;
}
}  // namespace

int mj_replay_load_pool(MjPool* dst, MjPool* src, int table0, const uint8_t* tracked_host, int always_include_kan_select,
                        int flags, int64_t counts_out[3], void* stream) {
    if (!dst || !src) return fail("null pool");
    if (!counts_out) return fail("mj_replay_load_pool: null counts buffer");
    memset(counts_out, 0, 3 * sizeof(int64_t));
    if (src == dst) return fail("mj_replay_load_pool: the source pool cannot be its own destination (the load restarts the destination's tables)");
    LogSrc S;
    if (pool_log_src("mj_replay_load_pool", src, table0, dst->n_tables, (hipStream_t)stream, S, "mj_replay_load_harvest loads",
                     "the event log of the source pool"))
        return -1;
    return replay_load_src("mj_replay_load_pool", dst, S, SeedSrc{src->blocks.get(), table0, nullptr, nullptr}, tracked_host,
                           always_include_kan_select, flags, counts_out, (hipStream_t)stream);
}

// Packed host logs through the augmenting copy and back (the pack walk of the loads above, over concatenated logs).  The three
// passes compact the accepted logs; the host puts each back at its own offsets, a malformed one stays as it came.
int mj_augment_logs(const uint64_t* words_host, const uint32_t* off_host, int n_logs, uint64_t* words_out_host, int64_t counts_out[3],
                    void* stream) {
    if (!counts_out) return fail("mj_augment_logs: null counts buffer");
    memset(counts_out, 0, 3 * sizeof(int64_t));
    hipStream_t s = (hipStream_t)stream;
    HostLogs L;
    if (upload_logs("mj_augment_logs", words_host, off_host, n_logs, s, L)) return -1;
    if (!L.src.n_logs) return 0;
    const size_t n_words = off_host[n_logs], n = (size_t)n_logs;
    if (n_words && !words_out_host) return fail("mj_augment_logs: null words");
    DevBuf<uint64_t> b_out;
    DevBuf<uint32_t> b_len, b_pack;     // b_pack: the compacted offsets [n + 1]
    DevBuf<unsigned long long> b_sums;  // done / empty / malformed, total words
    if (b_out.alloc(n_words + 1) || b_len.alloc(n) || b_pack.alloc(n + 1) || b_sums.alloc(4)) return -1;
    HIP_OK(hipMemsetAsync(b_sums.get(), 0, 4 * sizeof(unsigned long long), s));
    auto whole = [&](uint64_t*& out) { return out = b_out.get(), 0; };  // (an accepted log's length is its own: never more than n_words)
    if (log_pack_run(L.src, b_len.get(), b_pack.get(), b_sums.get(), whole, true, 0, s)) return -1;
    std::vector<uint32_t> len(n);
    std::vector<uint64_t> packed(n_words);
    unsigned long long sums_host[4];
    HIP_OK(hipMemcpyAsync(len.data(), b_len.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (n_words) HIP_OK(hipMemcpyAsync(packed.data(), b_out.get(), n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(sums_host, b_sums.get(), sizeof sums_host, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t lo = off_host[i], k = off_host[i + 1] - lo;
        if (len[i] == k && k) memcpy(words_out_host + lo, packed.data() + at, k * sizeof(uint64_t)), at += k;
        else if (k) memmove(words_out_host + lo, words_host + lo, k * sizeof(uint64_t));
    }
    for (int k = 0; k < 3; k++) counts_out[k] = (int64_t)sums_host[k];
    return 0;
}

// ---------------------------------------------------------------- finished games of a refilling pool (mj_harvest.hip)
struct MjHarvest {
    HarvestBuf buf;                    // the detached buffer: records in arrival order, words
    std::vector<MjHarvestGame> games;  // the records sorted by (game_id, table); the arrays below are in this order
    DevBuf<uint64_t> start, nonce, key;
    DevBuf<uint32_t> len;
    DevBuf<uint8_t> group;             // agent_of_seat
    int64_t n_words = 0, dropped = 0, n_err = 0;
};

int mj_pool_enable_harvest(MjPool* P, uint32_t max_games, uint64_t max_words) {
    if (!P) return fail("null pool");
    if (!P->log) return fail("mj_pool_enable_harvest: the event log is not enabled (mj_pool_enable_log)");
    hipStream_t s = P->step_stream;
    HarvestBuf B;  // (max_games 0: none -- harvesting is turned off)
    if (max_games && B.alloc(max_games, max_words & ~1ull, s)) return -1;
    HIP_OK(hipStreamSynchronize(s));  // behind the steps that may still be writing the buffer that goes
    P->hv = std::move(B);
    return 0;
}

int mj_harvest_pending(MjPool* P, int64_t out[3], void* stream) {
    if (!P || !out) return fail("null pool / output");
    if (!P->hv.games) return fail("mj_harvest_pending: harvesting is not enabled (mj_pool_enable_harvest)");
    hipStream_t s = (hipStream_t)stream;
    if (wait_snapshot(P, s)) return -1;
    unsigned long long c[HV_CURSORS];
    HIP_OK(hipMemcpyAsync(c, P->hv.cursors.get(), sizeof c, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    out[0] = (int64_t)c[HV_GAMES], out[1] = (int64_t)c[HV_WORDS], out[2] = (int64_t)c[HV_DROPPED];
    return 0;
}

int mj_harvest_take(MjPool* P, MjHarvest** out, void* stream) {
    if (!P || !out) return fail("null pool / output");
    *out = nullptr;
    if (!P->hv.games) return fail("mj_harvest_take: harvesting is not enabled (mj_pool_enable_harvest)");
    hipStream_t s = (hipStream_t)stream;
    if (wait_snapshot(P, s)) return -1;  // behind the last step, whatever its stream
    // the replacement first; the pool keeps its buffer until nothing can fail any more
    HarvestBuf fresh;
    if (fresh.alloc(P->hv.max_games, P->hv.max_words, s)) return -1;
    std::unique_ptr<MjHarvest> H(new MjHarvest);
    unsigned long long c[HV_CURSORS];
    HIP_OK(hipMemcpyAsync(c, P->hv.cursors.get(), sizeof c, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    const size_t n = (size_t)std::min<unsigned long long>(c[HV_GAMES], P->hv.max_games);
    H->games.resize(n);
    if (n) HIP_OK(hipMemcpyAsync(H->games.data(), P->hv.games.get(), n * sizeof(MjHarvestGame), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::sort(H->games.begin(), H->games.end(), [](const MjHarvestGame& a, const MjHarvestGame& b) {
        return a.game_id != b.game_id ? a.game_id < b.game_id : a.table < b.table;
    });
    std::vector<uint64_t> start(n), nonce(n), key(n);
    std::vector<uint32_t> len(n);
    std::vector<uint8_t> group(n);
    for (size_t i = 0; i < n; i++) {
        const MjHarvestGame& g = H->games[i];
        if (g.first_word > P->hv.max_words || g.n_words > P->hv.max_words - g.first_word)
            return fail("mj_harvest_take: record " + std::to_string(i) + " points outside the buffer");
        start[i] = g.first_word, len[i] = g.n_words, nonce[i] = g.seed_nonce, key[i] = g.seed_key, group[i] = g.agent_of_seat;
        H->n_words += g.n_words;
        H->n_err += g.err != 0;
    }
    H->dropped = (int64_t)c[HV_DROPPED];
    if (stat_upload(H->start, start.data(), n, s) || stat_upload(H->len, len.data(), n, s) || stat_upload(H->nonce, nonce.data(), n, s) ||
        stat_upload(H->key, key.data(), n, s) || stat_upload(H->group, group.data(), n, s))
        return -1;
    HIP_OK(hipStreamSynchronize(s));
    std::swap(P->hv, fresh);          // later steps write into the replacement ...
    H->buf = std::move(fresh);        // ... and the filled buffer leaves with the harvest
    *out = H.release();
    return 0;
}

void mj_harvest_destroy(MjHarvest* h) { delete h; }

int mj_harvest_info(const MjHarvest* h, int64_t out[4]) {
    if (!h || !out) return fail("null harvest / output");
    out[0] = (int64_t)h->games.size(), out[1] = h->n_words, out[2] = h->dropped, out[3] = h->n_err;
    return 0;
}
int mj_harvest_games(const MjHarvest* h, MjHarvestGame* host_out) {
    if (!h) return fail("null harvest");
    if (h->games.size() && !host_out) return fail("mj_harvest_games: null output");
    if (h->games.size()) memcpy(host_out, h->games.data(), h->games.size() * sizeof(MjHarvestGame));
    return 0;
}
int mj_harvest_read(const MjHarvest* h, int game, uint64_t* words_out) {
    if (!h) return fail("null harvest");
    if (game < 0 || (size_t)game >= h->games.size()) return fail("mj_harvest_read: game " + std::to_string(game) + " is not in the harvest");
    const MjHarvestGame& g = h->games[game];
    if (g.n_words == 0) return 0;
    if (!words_out) return fail("mj_harvest_read: null output");
    HIP_OK(hipMemcpy(words_out, h->buf.words.get() + g.first_word, (size_t)g.n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

namespace {
LogSrc harvest_log_src(const MjHarvest* h, int game0, int n) {
    LogSrc S{};
    S.words = h->buf.words.get();
    S.start = h->start.get() + game0;
    S.len = h->len.get() + game0;
    S.n_logs = n;
    return S;
}
}  // namespace

int mj_harvest_stat(const MjHarvest* h, const uint8_t* seats_host, int64_t* totals_out, int64_t* per_seat_out, int64_t counts_out[3],
                    void* stream) {
    if (!h) return fail("null harvest");
    if (stat_args(totals_out, counts_out)) return -1;
    if (h->games.empty()) return 0;
    StatParams K{};
    K.src = harvest_log_src(h, 0, (int)h->games.size());
    K.groups = h->group.get();
    return stat_run(K, seats_host, totals_out, per_seat_out, counts_out, (hipStream_t)stream);
}

int mj_harvest_grp(const MjHarvest* h, int game0, int n, int max_kyoku, int32_t* feat_out, int32_t* n_kyoku_out, int32_t* rank_out,
                   int32_t* final_out, int64_t counts_out[3], void* stream) {
    if (!h) return fail("null harvest");
    if (grp_args("mj_harvest_grp", n, max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out)) return -1;
    if (game0 < 0 || game0 > (int)h->games.size() - n) return fail("mj_harvest_grp: game range out of bounds");
    if (n == 0) return 0;
    return grp_run(harvest_log_src(h, game0, n), max_kyoku, feat_out, n_kyoku_out, rank_out, final_out, counts_out, (hipStream_t)stream);
}

int mj_replay_load_harvest(MjPool* dst, const MjHarvest* h, int game0, const uint8_t* tracked_host, int always_include_kan_select,
                           int flags, int64_t counts_out[3], void* stream) {
    if (!dst || !h) return fail("null pool / harvest");
    if (!counts_out) return fail("mj_replay_load_harvest: null counts buffer");
    memset(counts_out, 0, 3 * sizeof(int64_t));
    const int n = dst->n_tables;
    if (game0 < 0 || game0 > (int)h->games.size() - n) return fail("mj_replay_load_harvest: game range out of bounds");
    return replay_load_src("mj_replay_load_harvest", dst, harvest_log_src(h, game0, n),
                           SeedSrc{nullptr, 0, h->nonce.get() + game0, h->key.get() + game0}, tracked_host, always_include_kan_select,
                           flags, counts_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------- sample store (mj_samples.hip)
struct MjSamples {
    int64_t capacity = 0, count = 0;
    int version = 0, batch_rows = 0;
    DevBuf<TableOne> rec;    // [capacity] a sample's record ...
    DevBuf<uint32_t> desc;   // ... its row descriptor without the table (seat, kan flag) ...
    DevBuf<int32_t> meta;    // ... and its eight int32 of mj_k_replay_meta, [1] = the game number
    // The indices of the encode call under way: copied to pinned memory (the caller's array may go when the call returns), from there
    // to the device in one copy; ev_idx, recorded behind that copy, is what the next call waits for before it overwrites the pinned words.
    DevBuf<int32_t> idx;     // [idx_cap]
    PinnedBuf<int32_t> idx_pin;
    Event ev_idx;
    int idx_cap = 0;         // batch_rows at first, grown to the largest call
    // The encode context: a pool of batch_rows tables that is never stepped.  The encode launches take from it what they take from
    // a pool beside the records -- obs version, op-list flag, SP resources, knobs, timers -- and its rows[0] holds a chunk's descriptors.
    std::unique_ptr<MjPool> ctx;
    hipStream_t enc_stream = nullptr;  // the stream of the last encode: mj_samples_info reads the overflow words behind it
};
#define MJ_SAMPLES_MAX ((int64_t)ROW_TABLE(~0u))  // a sample's index is the ROW_TABLE field of its row: 2^28 - 1

MjSamples* mj_samples_create(int64_t capacity, int version, int batch_rows) {
    if (capacity < 1 || capacity > MJ_SAMPLES_MAX) {
        fail("mj_samples_create: capacity " + std::to_string(capacity) + " is not in [1, " + std::to_string(MJ_SAMPLES_MAX) +
             "] (a sample's index takes the 28 table bits of a row descriptor)");
        return nullptr;
    }
    if (batch_rows < 1) {
        fail("mj_samples_create: batch_rows must be at least 1");
        return nullptr;
    }
    std::unique_ptr<MjSamples> S(new MjSamples);
    S->ctx.reset(mj_pool_create(batch_rows, version, MJ_DEAL_RAND08, batch_rows));  // (refuses a bad version, missing tables)
    if (!S->ctx) return nullptr;
    if (S->rec.alloc((size_t)capacity) || S->desc.alloc((size_t)capacity) || S->meta.alloc((size_t)capacity * 8) ||
        S->idx.alloc((size_t)batch_rows) || S->idx_pin.alloc((size_t)batch_rows) || S->ev_idx.create_no_timing())
        return nullptr;
    S->idx_cap = batch_rows;
    S->capacity = capacity;
    S->version = version;
    S->batch_rows = batch_rows;
    return S.release();
}

void mj_samples_destroy(MjSamples* S) { delete S; }

int mj_samples_append(MjSamples* S, MjPool* P, int32_t log_base, void* stream) {
    if (!S || !P) return fail("null store / pool");
    if (!P->rp.script) return fail("mj_samples_append: the pool has no replay script (the label of a sample comes from it): mj_replay_load first");
    if (!P->rows_valid) return fail("mj_rows_count must be called after mj_replay_step and before mj_samples_append");
    const int n = P->last_rows[0];
    if (n == 0) return 0;
    if (S->count + n > S->capacity)
        return fail("mj_samples_append: " + std::to_string(n) + " rows do not fit a store of " + std::to_string(S->capacity) +
                    " samples that holds " + std::to_string(S->count));
    hipStream_t s = (hipStream_t)stream;
    if (wait_snapshot(P, s)) return -1;
    const SamplesAppendParams ap = {P->snap.get(), P->blocks.get(), P->rows[0].get(), n, P->rp.label.get(), P->rp.kan_label.get(),
                                    P->rp.kyoku.get(), P->rp.ev_index.get(), log_base, S->rec.get() + S->count,
                                    S->desc.get() + S->count, S->meta.get() + S->count * 8};
    hipLaunchKernelGGL(mj_k_samples_append, dim3(n), dim3(64), 0, s, ap);
    HIP_OK(hipGetLastError());
    S->count += n;
    return 0;
}

int mj_samples_truncate(MjSamples* S, int64_t count) {
    if (!S) return fail("null store");
    if (count < 0 || count > S->count)
        return fail("mj_samples_truncate: " + std::to_string(count) + " is not in [0, " + std::to_string(S->count) + "]");
    S->count = count;
    return 0;
}

int mj_samples_info(const MjSamples* S, int64_t out[4]) {
    if (!S || !out) return fail("null store / output");
    out[0] = S->count, out[1] = S->capacity, out[2] = (int64_t)(sizeof(TableOne) + sizeof(uint32_t) + 8 * sizeof(int32_t)), out[3] = 0;
    HIP_OK(hipStreamSynchronize(S->enc_stream));
    int f = 0;
    HIP_OK(hipMemcpy(&f, S->ctx->enc_flag.get(), sizeof f, hipMemcpyDeviceToHost));
    out[3] = f;
    if (S->ctx->sp.err) {
        unsigned long long ov = 0;
        HIP_OK(hipMemcpy(&ov, S->ctx->sp.err.get() + SP_ERR_OVERFLOW, sizeof ov, hipMemcpyDeviceToHost));
        out[3] += (int64_t)ov;
    }
    return 0;
}

int mj_samples_meta(const MjSamples* S, int64_t first, int64_t n, int32_t* meta_host, void* stream) {
    if (!S) return fail("null store");
    if (first < 0 || n < 0 || first > S->count - n) return fail("mj_samples_meta: sample range out of bounds");
    if (n == 0) return 0;
    if (!meta_host) return fail("mj_samples_meta: null output");
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(meta_host, S->meta.get() + first * 8, (size_t)n * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

namespace {
// Every index checked before anything is queued; then the indices to the device and per chunk of batch_rows: their descriptors into
// the context's row list, `launch(source, rows of the chunk, first row of the chunk)`.
int samples_chunks(const char* who, MjSamples* S, const int32_t* idx_host, int n, hipStream_t s,
                   const std::function<int(const EncSrc&, int, int64_t)>& launch) {
    if (!S) return fail("null store");
    if (n < 0) return fail(std::string(who) + ": negative number of samples");
    if (n == 0) return 0;
    if (!idx_host) return fail(std::string(who) + ": null indices");
    for (int i = 0; i < n; i++)
        if (idx_host[i] < 0 || idx_host[i] >= S->count)
            return fail(std::string(who) + ": index " + std::to_string(idx_host[i]) + " (position " + std::to_string(i) +
                        ") is not in a store of " + std::to_string(S->count) + " samples");
    HIP_OK(hipEventSynchronize(S->ev_idx.get()));  // the last call's copy out of the pinned words
    if (n > S->idx_cap) {
        DevBuf<int32_t> idx;
        PinnedBuf<int32_t> pin;
        if (idx.alloc((size_t)n) || pin.alloc((size_t)n)) return -1;
        S->idx = std::move(idx);  // (the smaller pair goes with the locals; hipFree waits for the kernels that read it)
        S->idx_pin = std::move(pin);
        S->idx_cap = n;
    }
    memcpy(S->idx_pin.get(), idx_host, (size_t)n * sizeof(int32_t));
    HIP_OK(hipMemcpyAsync(S->idx.get(), S->idx_pin.get(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(S->ev_idx.get(), s));
    uint32_t* rows = S->ctx->rows[0].get();
    const EncSrc src = {S->rec.get(), rows};
    S->enc_stream = s;
    for (int64_t at = 0; at < n; at += S->batch_rows) {
        const int k = (int)std::min<int64_t>(S->batch_rows, n - at);
        hipLaunchKernelGGL(mj_k_samples_rows, dim3((k + 255) / 256), dim3(256), 0, s, S->idx.get() + at, S->desc.get(), k, rows);
        HIP_OK(hipGetLastError());
        if (launch(src, k, at)) return -1;
    }
    return 0;
}
}  // namespace

int mj_samples_encode(MjSamples* S, const int32_t* idx_host, int n, float* obs, uint8_t* masks, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t row = S ? (size_t)mj_obs_rows(S->version) * 34 : 0;
    return samples_chunks("mj_samples_encode", S, idx_host, n, s, [&](const EncSrc& src, int k, int64_t at) {
        return encode_launch(S->ctx.get(), 0, src, k, obs + (size_t)at * row, masks + (size_t)at * 46, s);
    });
}

int mj_samples_encode_oracle(MjSamples* S, const int32_t* idx_host, int n, float* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t row = S ? (size_t)mj_oracle_obs_rows(S->version) * 34 : 0;
    return samples_chunks("mj_samples_encode_oracle", S, idx_host, n, s, [&](const EncSrc& src, int k, int64_t at) {
        return encode_oracle_launch(S->version, src, k, out + (size_t)at * row, 1 /* the sources are replay pools */, s);
    });
}

__global__ void mj_k_first_error(const TableBlock* blocks, int n_tables, unsigned long long* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tables) return;
    const unsigned e = blocks[t >> 6].err[t & 63];
    if (e) atomicMin(out, ((unsigned long long)t << 8) | e);
}
int mj_pool_first_error(MjPool* P, int* table_out, void* stream) {
    if (!P) return fail("null pool");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* slot = P->counters.get() + 7;  // spare counter word
    HIP_OK(hipMemsetAsync(slot, 0xFF, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(mj_k_first_error, dim3((P->n_tables + 255) / 256), dim3(256), 0, s, P->blocks.get(), P->n_tables, slot);
    HIP_OK(hipGetLastError());
    unsigned long long v = 0;
    HIP_OK(hipMemcpyAsync(&v, slot, sizeof v, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (v == ~0ull) return 0;
    if (table_out) *table_out = (int)(v >> 8);
    return (int)(v & 0xFF);
}

int mj_debug_table(MjPool* P, int table, void* out, size_t out_size, void* stream) {
    if (!P || table < 0 || table >= P->n_tables) return fail("bad table");
    if (out_size < sizeof(TableOne)) return fail("buffer too small");
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    std::vector<uint8_t> blk(sizeof(TableBlock));
    HIP_OK(hipMemcpy(blk.data(), &P->blocks.get()[table >> 6], sizeof(TableBlock), hipMemcpyDeviceToHost));
    auto g = build_gather();
    int lane = table & 63;
    for (auto& e : g) memcpy((char*)out + e.dst_off, blk.data() + e.src_off + (size_t)lane * e.size, e.size);
    return 0;
}

}  // extern "C"
