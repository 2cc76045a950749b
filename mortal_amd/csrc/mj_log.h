// Reading packed event logs (mj_state.h LG_* words) on the device: the one definition of where a log lies, how long an event is,
// how its chain is walked, how the running scores end as a ranking, and how a kernel reports its three counts.  Shared by
// mj_k_log_stat (mj_stat.hip), mj_k_log_len / mj_k_log_pack / mj_k_log_grp (mj_gameplay.hip) and mj_k_replay (mj_replay.hip).
//
// Shape of every kernel over logs: one wavefront handles one log at a time, grid-stride over the logs.  A log is a chain of events
// from word 0 (a payload word can look like any header), so the chain is walked in order; what is spread over the wavefront is the
// memory access: the 64 lanes load 64 consecutive words as one coalesced 512-byte read, and every word the walk needs is then
// taken from a lane's register with a wave-uniform __shfl -- no lane streams a log of its own, nothing is staged in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mj_algo.h"

// the one grid rule (mj_capi.hip log_grid; MJ_LOG_GRID lowers the grid: tests)
#define LOG_WAVES 4                 // wavefronts (= logs in flight) per workgroup
#define LOG_THREADS (64 * LOG_WAVES)
#define LOG_GRID_MAX (256 * 4)      // bounded grid: four workgroups per CU of a 256-CU device, the rest by grid stride
#define LOG_WINDOW_LAST 60          // log_walk_events: header + tag + two payload words <= window index 63

// The three addressings: concatenated logs with `off`, tables [table0, table0 + n_logs) of a pool's strided log, or scattered logs
// of a harvest (mj_harvest.hip) with `start`.
struct LogSrc {
    const uint64_t* words;
    const uint32_t* off;         // [n_logs + 1], or NULL: log i is table table0 + i, at words + table * stride ...
    const uint32_t* len;         // ... with len[table] words
    uint32_t stride;
    const TableBlock* blocks;    // pool path: flags / err / agent_of_seat of the table; NULL otherwise
    int table0;
    int n_logs;
    const uint64_t* start;       // [n_logs], or NULL; scattered: log i is words + start[i] with len[i] words, len[i] == 0 = skipped
};
enum { LOG_OK = 0, LOG_SKIP = 1, LOG_BAD = 2 };

// log i -> its words and length; LOG_SKIP: nothing to read (an empty log; a table whose game has not finished without an error),
// LOG_BAD: log_len beyond log_cap.  That branch cannot be reached for a table with err == MJ_OK: the push that overflows a log
// sets MJ_ERR_LOG_OVERFLOW (mj_rules.h log_push), and a table in error is skipped one line earlier.
MJD int log_locate(const LogSrc& S, int i, const uint64_t*& lw, uint32_t& len) {
    if (S.off) {
        lw = S.words + (size_t)S.off[i];
        len = S.off[i + 1] - S.off[i];
        return len ? LOG_OK : LOG_SKIP;
    }
    if (S.start) {
        lw = S.words + (size_t)S.start[i];
        len = S.len[i];
        return len ? LOG_OK : LOG_SKIP;
    }
    const int t = S.table0 + i;
    lw = S.words + (size_t)t * S.stride;
    len = S.len[t];
    const TableBlock* B = S.blocks + (t >> 6);
    const uint32_t fl = B->flags[t & 63];
    if (!(fl & TF_DONE) || (fl & TF_INACTIVE) || B->err[t & 63] != MJ_OK || len == 0) return LOG_SKIP;
    return len > S.stride ? LOG_BAD : LOG_OK;
}

// words of the event whose header is (w_lo, w_hi): a function of the header alone (arena logs carry one tag word per decision)
MJD int log_event_len(uint32_t w_lo, uint32_t w_hi) {
    const int t = w_lo & 15;
    if (t == LG_START_KYOKU) return (w_hi >> (LG_SK_WALL_BIT - 32)) & 1 ? 27 : 10;
    return (t == LG_HORA ? 4 : t == LG_RYUKYOKU ? 3 : 1) + (int)((w_hi >> (LG_TAG_BIT - 32)) & 1);
}

// the header at index k (wave-uniform) of the window the lanes hold in `mine` -> it is a known event's
MJD bool log_header(uint64_t mine, int k, uint32_t& w_lo, uint32_t& w_hi) {
    const uint64_t wv = __shfl(mine, k);
    w_lo = __builtin_amdgcn_readfirstlane((uint32_t)wv);
    w_hi = __builtin_amdgcn_readfirstlane((uint32_t)(wv >> 32));
    const int t = w_lo & 15;
    return !(t < LG_START_KYOKU || t > LG_END_KYOKU);
}

MJD int log_pick(int s, int v0, int v1, int v2, int v3) { return s == 0 ? v0 : s == 1 ? v1 : s == 2 ? v2 : v3; }

struct LogEvent {             // one event as log_walk_events hands it over (wave-uniform)
    uint32_t w_lo, w_hi;      // the header word
    int type, actor, target;
    int d0, d1, d2, d3;       // start_kyoku: scores; hora / ryukyoku: deltas; any other event: what the last of those left
};
// The four scores as the events move them (wave-uniform): a start_kyoku sets them, hora / ryukyoku add their deltas, reach_accepted
// takes 1000 -- what stands at the end is what the reference collects backwards up to the last start_kyoku (dataset/grp.rs:90-164).
struct LogScores {
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    MJD void apply(const LogEvent& e) {  // (an event of any other type moves nothing)
        if (e.type == LG_START_KYOKU) {
            c0 = e.d0, c1 = e.d1, c2 = e.d2, c3 = e.d3;
        } else if (e.type == LG_HORA || e.type == LG_RYUKYOKU) {
            c0 += e.d0, c1 += e.d1, c2 += e.d2, c3 += e.d3;
        } else if (e.type == LG_REACH_ACCEPTED) {
            c0 -= e.actor == 0 ? 1000 : 0, c1 -= e.actor == 1 ? 1000 : 0;
            c2 -= e.actor == 2 ? 1000 : 0, c3 -= e.actor == 3 ? 1000 : 0;
        }
    }
    // Rankings::new for seat `pid`: stable, ties to the lower seat; the top-up to 100,000 goes to first place after ranking
    MJD void final_of(int pid, int& rank, int& final_score) const {
        const int mine = log_pick(pid, c0, c1, c2, c3);
        rank = (c0 > mine || (c0 == mine && 0 < pid)) + (c1 > mine || (c1 == mine && 1 < pid)) +
               (c2 > mine || (c2 == mine && 2 < pid)) + (c3 > mine || (c3 == mine && 3 < pid));
        const int total = c0 + c1 + c2 + c3;
        final_score = mine + (rank == 0 && total < 100000 ? 100000 - total : 0);
    }
};

// The walk that reads payloads: every event of the log in order, handed to `on_event(const LogEvent&) -> bool` (false: malformed)
// with `sc` already moved by it; everything handed over is wave-uniform.  A window is left as soon as an event's header, tag and
// first two payload words could lie outside it, and the next window starts at that event, so payloads that straddle a 64-word
// boundary need no case of their own.  -> the chain is a sequence of known events that ends exactly at `len`.
template <class F>
MJD bool log_walk_events(const uint64_t* lw, uint32_t len, int lane, LogScores& sc, F&& on_event) {
    uint32_t pos = 0;
    LogEvent e{};  // (outside the loops: an event without a payload costs no write of d0..d3)
    while (pos < len) {
        const uint32_t base = pos;
        const uint64_t mine = base + (uint32_t)lane < len ? lw[base + lane] : 0ull;  // never beyond len
        while (pos < len && pos - base <= LOG_WINDOW_LAST) {
            const int k = __builtin_amdgcn_readfirstlane((int)(pos - base));
            if (!log_header(mine, k, e.w_lo, e.w_hi)) return false;
            const uint32_t next = pos + (uint32_t)log_event_len(e.w_lo, e.w_hi);
            if (next > len) return false;  // the chain runs past the end of the log
            pos = next;
            e.type = e.w_lo & 15, e.actor = (e.w_lo >> 4) & 3, e.target = (e.w_lo >> 6) & 3;
            if (e.type == LG_START_KYOKU || e.type == LG_HORA || e.type == LG_RYUKYOKU) {
                const int p = k + 1 + (e.type != LG_START_KYOKU ? (int)((e.w_hi >> (LG_TAG_BIT - 32)) & 1) : 0);  // first payload word
                const uint64_t a = __shfl(mine, p), b = __shfl(mine, p + 1);
                e.d0 = (int)(uint32_t)a, e.d1 = (int)(uint32_t)(a >> 32), e.d2 = (int)(uint32_t)b, e.d3 = (int)(uint32_t)(b >> 32);
                sc.apply(e);
            } else if (e.type == LG_REACH_ACCEPTED) {
                sc.apply(e);
            }
            if (!on_event(e)) return false;
        }
    }
    return true;
}

// ok / skipped / malformed logs of one wavefront, and their flush: one atomicAdd per non-zero count and wavefront
struct LogCounts {
    unsigned n_ok = 0, n_skip = 0, n_bad = 0;
    MJD void add(int st) { n_ok += st == LOG_OK, n_skip += st == LOG_SKIP, n_bad += st == LOG_BAD; }
    MJD unsigned of_lane(int lane) const { return lane == 0 ? n_ok : lane == 1 ? n_skip : n_bad; }  // one count per lane
    MJD void flush(int lane, unsigned long long* counts) const {
        const unsigned n_mine = of_lane(lane);
        if (lane < 3 && n_mine) atomicAdd(&counts[lane], (unsigned long long)n_mine);
    }
};
