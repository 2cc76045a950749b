// Finished games collected from a pool in refill mode (the reference hands each GameResult over as its game finishes,
// arena/game.rs:291-296, and keeps seed, scores and log with it, arena/result.rs:19-51).  mj_k_refill rewinds a finished table's log
// in the step after the one that finished it; mj_k_harvest runs directly in front of it and copies what is about to be rewound --
// the log's words, the seed, the final scores -- into the pool's harvest buffer.  The reducers (mj_k_log_stat, mj_k_log_grp) and
// the replay loader then read the buffer through the scattered addressing of LogSrc (mj_log.h).
//
// Shape, as mj_k_refill: one 64-lane workgroup per TableBlock.  The wavefront ballots the lanes whose table is about to be restarted
// and loops over the set bits wave-uniformly; for each game its own lane reserves a word range and a record slot on the buffer's two
// cursors, then all 64 lanes copy the log as coalesced reads and writes.  A reservation is an even number of words, so both sides of
// the copy are 16-byte aligned when the log's stride is even and a lane moves 16 bytes at a time, HV_DEPTH of them in flight (a log
// of ~3,000 words is copied by one wavefront: what it costs is load latency, not bandwidth).  No lane streams a log of its own.
// A game that does not fit is dropped and counted: a reservation either succeeds whole or changes nothing (compare-and-swap against
// the capacity), so nothing is overwritten and the kernel never waits.  The order of the records is whatever the reservations'
// race gives; the host sorts them (mj_capi.hip mj_harvest_take).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mortal_amd.h"
#include "mj_algo.h"

static_assert(sizeof(MjHarvestGame) == 64, "MjHarvestGame layout");

#ifndef HV_DEPTH
#define HV_DEPTH 8  // 16-byte loads a lane issues before it stores them (8 KB per wavefront and round); -DHV_DEPTH=1: one at a time (A/B builds)
#endif
enum { HV_GAMES = 0, HV_WORDS = 1, HV_DROPPED = 2, HV_CURSORS = 4 };  // words of HarvestParams::cursors

struct HarvestParams {
    const TableBlock* blocks;
    int n_tables;
    uint32_t cycle;              // the step's cycle index, as mj_k_refill sees it
    uint32_t start_stagger;
    const uint64_t* log;         // [n_tables][log_cap]
    const uint32_t* log_len;
    uint32_t log_cap;
    MjHarvestGame* games;        // [max_games]
    uint64_t* words;             // [max_words]
    unsigned long long* cursors; // [HV_CURSORS]: records written, words reserved, games dropped
    unsigned long long max_games, max_words;
};

struct alignas(16) HvPair {
    uint64_t a, b;
};

// cursor += n unless that would pass cap -> the old value, or ~0 when it does not fit (then nothing has changed)
MJD unsigned long long hv_reserve(unsigned long long* cursor, unsigned long long n, unsigned long long cap) {
    unsigned long long cur = *(volatile unsigned long long*)cursor;
    for (;;) {
        if (cur > cap || n > cap - cur) return ~0ull;
        const unsigned long long seen = atomicCAS(cursor, cur, cur + n);
        if (seen == cur) return cur;
        cur = seen;
    }
}

__global__ __launch_bounds__(64) void mj_k_harvest(HarvestParams P) {
    const int l = threadIdx.x, table = blockIdx.x * 64 + l;
    const TableBlock* B = P.blocks + blockIdx.x;
    const uint32_t fl = B->flags[l];
    // mj_k_refill's own test, plus TF_ENDED: a table parked by mj_k_park is done without having played
    bool take = table < P.n_tables && !(fl & TF_INACTIVE) && (fl & TF_DONE) && (fl & TF_ENDED);
    if (take && P.start_stagger && P.cycle < (((uint32_t)table * 2654435761u) >> 8) % P.start_stagger) take = false;
    const bool even_stride = (P.log_cap & 1u) == 0;
    for (unsigned long long m = __ballot(take); m; m &= m - 1) {
        const int d = __ffsll((long long)m) - 1;
        uint32_t n = 0;                 // words to copy (this game's lane only)
        unsigned long long first = 0;
        if (l == d) {
            const uint32_t len = P.log_len[table];
            const uint8_t err = B->err[l];
            n = err == MJ_OK && len <= P.log_cap ? len : 0u;  // a game in error keeps its record, not its words
            const unsigned long long need = ((unsigned long long)n + 1ull) & ~1ull;
            // a full record array is seen before any words are reserved; the slot is taken after the words, so a record never
            // points at words it does not own (a slot lost to a race in between leaves an unused word range, nothing else)
            bool ok = *(volatile unsigned long long*)&P.cursors[HV_GAMES] < P.max_games;
            if (ok && need) {
                first = hv_reserve(&P.cursors[HV_WORDS], need, P.max_words);
                ok = first != ~0ull;
            }
            const unsigned long long slot = ok ? hv_reserve(&P.cursors[HV_GAMES], 1ull, P.max_games) : ~0ull;
            if (slot == ~0ull) {
                atomicAdd(&P.cursors[HV_DROPPED], 1ull);
                n = 0;
                first = 0;
            } else {
                MjHarvestGame g;
                g.seed_nonce = B->seed_nonce[l];
                g.seed_key = B->seed_key[l];
                g.first_word = first;
                g.n_words = n;
                g.game_id = B->game_id[l];
                g.table = (uint32_t)table;
                g.cycle = P.cycle;
                for (int i = 0; i < 4; i++) g.scores[i] = B->scores[i][l];
                g.err = err;
                g.agent_of_seat = B->agent_of_seat[l];
                for (int i = 0; i < 6; i++) g.reserved[i] = 0;
                P.games[slot] = g;
            }
        }
        const uint32_t n_all = __shfl(n, d);
        if (n_all == 0) continue;  // wave-uniform
        const unsigned long long first_all = __shfl(first, d);
        const uint64_t* src = P.log + (size_t)(blockIdx.x * 64 + d) * P.log_cap;
        uint64_t* dst = P.words + first_all;
        if (even_stride) {  // both sides 16-byte aligned: the stride and every reservation are even
            const HvPair* s2 = (const HvPair*)src;
            HvPair* d2 = (HvPair*)dst;
            const uint32_t n2 = n_all / 2;
            uint32_t k = l;
            for (; k + 64 * (HV_DEPTH - 1) < n2; k += 64 * HV_DEPTH) {  // HV_DEPTH loads in flight per lane, then their stores: one
                HvPair v[HV_DEPTH];                                     // wavefront copies a whole log, its time is load latency
#pragma unroll
                for (int j = 0; j < HV_DEPTH; j++) v[j] = s2[k + 64 * j];
#pragma unroll
                for (int j = 0; j < HV_DEPTH; j++) d2[k + 64 * j] = v[j];
            }
            for (; k < n2; k += 64) d2[k] = s2[k];
            if ((n_all & 1u) && l == 0) dst[n_all - 1] = src[n_all - 1];
        } else {
            for (uint32_t k = l; k < n_all; k += 64) dst[k] = src[k];
        }
    }
}
