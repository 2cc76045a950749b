// libriichi's Stat on the device: mj_k_log_stat reduces packed event logs (mj_state.h LG_* words) to the 44 counters of
// `Stat` (stat.rs:30-126), event by event as Stat::from_game does (stat.rs:263-441; host reading: mortal_amd/stat.py).
// Field order: include/mortal_amd.h MjStatField.
//
// Shape: one wavefront reduces one log at a time, grid-stride over the logs.  A log is a chain of events from word 0 (a
// payload word can look like any header), so the chain is walked in order; what is spread over the wavefront is the memory
// access: the 64 lanes load the 64 words that follow the chain position as one coalesced 512-byte read, and every word the
// walk needs is then taken from a lane's register with a wave-uniform __shfl -- no lane streams a log of its own, nothing
// is staged in LDS.  A window is left as soon as an event's header, tag and first two payload words (all Stat reads) could
// lie outside it, and the next window starts at that event, so payloads that straddle a 64-word boundary need no case of
// their own.  The event header and the scores are wave-uniform; lanes 0..3 each follow one seat (jun, fuuro count, riichi
// declared / accepted, others' riichi) and own that seat's 44 counters in LDS.  A finished log is handed to lanes 0..43
// (one field each) that store the per-seat rows and add the selected seats to the wavefront's totals; the workgroup's four
// wavefronts are summed once at the end, one 64-bit atomicAdd per non-zero field and workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mortal_amd.h"
#include "mj_algo.h"

#define STAT_WAVES 4                 // wavefronts (= logs in flight) per workgroup
#define STAT_THREADS (64 * STAT_WAVES)
#define STAT_GRID_MAX (256 * 4)      // bounded grid: four workgroups per CU of a 256-CU device, the rest by grid stride
#define STAT_WINDOW_LAST 60          // last window index an event may start at: header + tag + two payload words <= index 63

struct StatParams {
    const uint64_t* words;       // base of the logs
    const uint32_t* off;         // [n_logs + 1] word offsets of concatenated logs, or NULL: log i starts at i * stride ...
    const uint32_t* len;         // ... and has len[i] words (clamped to stride: an overflowed log_len counts past log_cap)
    uint32_t stride;
    const TableBlock* blocks;    // pool path: flags / err / agent_of_seat of table i; NULL otherwise
    const uint8_t* seats;        // [n_logs] 4-bit seat masks, NULL = all four
    const uint8_t* groups;       // [n_logs] bit s = group of seat s, NULL = 0 (pool path: agent_of_seat)
    int n_logs;
    unsigned long long* totals;  // [2][MJ_STAT_FIELDS], added to
    long long* per_seat;         // NULL or [n_logs][4][MJ_STAT_FIELDS], every row written
    unsigned long long* counts;  // [3] logs reduced / skipped / malformed, added to
    const uint64_t* start;       // [n_logs], or NULL; scattered (off NULL): log i starts at start[i] and has len[i] words, 0 = skipped
};

MJD int stat_pick(int s, int v0, int v1, int v2, int v3) { return s == 0 ? v0 : s == 1 ? v1 : s == 2 ? v2 : v3; }

__global__ __launch_bounds__(STAT_THREADS) void mj_k_log_stat(StatParams P) {
    __shared__ long long s_cnt[STAT_WAVES][4][MJ_STAT_FIELDS];            // the current log's counters, per seat
    __shared__ long long s_tot[STAT_WAVES][2][MJ_STAT_FIELDS];            // the wavefront's totals, per group
    __shared__ unsigned s_n[STAT_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pid = lane & 3;  // (lanes >= 4 follow the walk for the collectives only)
    long long* const C = &s_cnt[wave][pid][0];
    long long* const flat = &s_cnt[wave][0][0];
    for (int i = lane; i < 2 * MJ_STAT_FIELDS; i += 64) (&s_tot[wave][0][0])[i] = 0;
    unsigned n_reduced = 0, n_skipped = 0, n_malformed = 0;

    for (int log = blockIdx.x * STAT_WAVES + wave; log < P.n_logs; log += gridDim.x * STAT_WAVES) {
        const uint64_t* lw;
        uint32_t len;
        uint32_t seats = P.seats ? P.seats[log] & 15u : 15u, groups = P.groups ? P.groups[log] : 0u;
        bool skip = false;
        if (P.off) {
            lw = P.words + (size_t)P.off[log];
            len = P.off[log + 1] - P.off[log];
        } else if (P.start) {
            lw = P.words + (size_t)P.start[log];
            len = P.len[log];
        } else {
            lw = P.words + (size_t)log * P.stride;
            len = min(P.len[log], P.stride);
        }
        if (P.blocks) {  // only a game that has finished without an error
            const TableBlock* B = P.blocks + (log >> 6);
            const uint32_t fl = B->flags[log & 63];
            skip = !(fl & TF_DONE) || (fl & TF_INACTIVE) || B->err[log & 63] != MJ_OK;
            groups = B->agent_of_seat[log & 63];
        }
        if (len == 0) skip = true;
        for (int i = lane; i < 4 * MJ_STAT_FIELDS; i += 64) flat[i] = 0;
        mj_team_sync<64>();

        bool bad = false;
        if (!skip) {
            int cur0 = 0, cur1 = 0, cur2 = 0, cur3 = 0, oya = 0;                      // wave-uniform
            bool declared = false, accepted = false, others_declared = false;       // this lane's seat
            int jun = 0, fuuro = 0;
            uint32_t pos = 0;
            while (pos < len && !bad) {
                const uint32_t base = pos;
                const uint64_t mine = base + (uint32_t)lane < len ? lw[base + lane] : 0ull;  // never beyond len
                while (pos < len && pos - base <= STAT_WINDOW_LAST) {
                    const int k = __builtin_amdgcn_readfirstlane((int)(pos - base));
                    const uint64_t wv = __shfl(mine, k);
                    const uint32_t w_lo = __builtin_amdgcn_readfirstlane((uint32_t)wv);
                    const uint32_t w_hi = __builtin_amdgcn_readfirstlane((uint32_t)(wv >> 32));
                    const int t = w_lo & 15, actor = (w_lo >> 4) & 3, target = (w_lo >> 6) & 3;
                    if (t < LG_START_KYOKU || t > LG_END_KYOKU) { bad = true; break; }
                    int p = k + 1;  // window index of the first payload word
                    if (t != LG_START_KYOKU && ((w_hi >> (LG_TAG_BIT - 32)) & 1)) p++;
                    const int n_pay = t == LG_START_KYOKU ? 9 + ((w_hi >> (LG_SK_WALL_BIT - 32)) & 1 ? 17 : 0)
                                    : t == LG_HORA ? 3 : t == LG_RYUKYOKU ? 2 : 0;
                    const uint32_t next = base + (uint32_t)p + (uint32_t)n_pay;
                    if (next > len) { bad = true; break; }  // the chain runs past the end of the log
                    pos = next;
                    int d0 = 0, d1 = 0, d2 = 0, d3 = 0;  // start_kyoku: scores; hora / ryukyoku: deltas
                    if (n_pay) {
                        const uint64_t a = __shfl(mine, p), b = __shfl(mine, p + 1);
                        d0 = (int)(uint32_t)a, d1 = (int)(uint32_t)(a >> 32), d2 = (int)(uint32_t)b, d3 = (int)(uint32_t)(b >> 32);
                    }
                    const bool seat_lane = lane < 4;
                    const bool me = actor == pid;
                    const bool is_oya = oya == pid;
                    switch (t) {
                        case LG_START_KYOKU:
                            cur0 = d0, cur1 = d1, cur2 = d2, cur3 = d3;
                            oya = (int)((w_lo >> 14) & 63) & 3;  // kyoku % 4 (the kyoku index 0..15 travels in c0)
                            declared = accepted = others_declared = false;
                            jun = fuuro = 0;
                            if (seat_lane) {
                                C[MJ_ST_ROUND] += 1;
                                if (oya == pid) C[MJ_ST_OYA] += 1;
                            }
                            break;
                        case LG_DAHAI:
                            if (me) jun++;
                            break;
                        case LG_CHI:
                        case LG_PON:
                        case LG_DAIMINKAN:
                            if (me) fuuro++;
                            break;
                        case LG_REACH:
                            if (me) {
                                declared = true;
                                if (seat_lane) {
                                    C[MJ_ST_RIICHI] += 1;
                                    C[MJ_ST_RIICHI_JUN] += jun;
                                    if (is_oya) C[MJ_ST_RIICHI_AS_OYA] += 1;
                                    if (others_declared) C[MJ_ST_CHASING_RIICHI] += 1;
                                }
                            } else if (declared) {
                                if (seat_lane) C[MJ_ST_RIICHI_GOT_CHASED] += 1;
                            } else {
                                others_declared = true;
                            }
                            break;
                        case LG_REACH_ACCEPTED:
                            cur0 -= actor == 0 ? 1000 : 0, cur1 -= actor == 1 ? 1000 : 0;
                            cur2 -= actor == 2 ? 1000 : 0, cur3 -= actor == 3 ? 1000 : 0;
                            if (me) accepted = true;
                            break;
                        case LG_HORA: {
                            cur0 += d0, cur1 += d1, cur2 += d2, cur3 += d3;
                            const int delta = stat_pick(pid, d0, d1, d2, d3);
                            if (!seat_lane) break;
                            if (me) {
                                const int point = delta - (accepted ? 1000 : 0);
                                C[MJ_ST_AGARI] += 1;
                                C[MJ_ST_AGARI_JUN] += jun;
                                if (is_oya) {
                                    C[MJ_ST_AGARI_AS_OYA] += 1;
                                    C[MJ_ST_AGARI_POINT_OYA] += point;
                                } else {
                                    C[MJ_ST_AGARI_POINT_KO] += point;
                                }
                                if (accepted) {
                                    C[MJ_ST_RIICHI_AGARI] += 1;
                                    C[MJ_ST_RIICHI_AGARI_JUN] += jun;
                                    C[MJ_ST_RIICHI_AGARI_POINT] += point;
                                    C[MJ_ST_RIICHI_POINT] += point;
                                } else if (fuuro > 0) {
                                    C[MJ_ST_FUURO_AGARI] += 1;
                                    C[MJ_ST_FUURO_AGARI_JUN] += jun;
                                    C[MJ_ST_FUURO_AGARI_POINT] += point;
                                    C[MJ_ST_FUURO_POINT] += point;
                                } else {
                                    C[MJ_ST_DAMA_AGARI] += 1;
                                    C[MJ_ST_DAMA_AGARI_JUN] += jun;
                                    C[MJ_ST_DAMA_AGARI_POINT] += point;
                                }
                                if (point >= (is_oya ? 48000 : 32000)) C[MJ_ST_YAKUMAN] += 1;  // Point::yakuman(is_oya, 1).ron
                            } else if (target == pid) {
                                C[MJ_ST_HOUJUU] += 1;
                                C[MJ_ST_HOUJUU_JUN] += jun;
                                if (oya == actor) {
                                    C[MJ_ST_HOUJUU_TO_OYA] += 1;
                                    C[MJ_ST_HOUJUU_POINT_TO_OYA] += delta;
                                } else {
                                    C[MJ_ST_HOUJUU_POINT_TO_KO] += delta;
                                }
                                if (declared) {
                                    C[MJ_ST_RIICHI_HOUJUU] += 1;
                                    C[MJ_ST_RIICHI_POINT] += delta;
                                } else if (fuuro > 0) {
                                    C[MJ_ST_FUURO_HOUJUU] += 1;
                                    C[MJ_ST_FUURO_POINT] += delta;
                                }
                            }
                            break;
                        }
                        case LG_RYUKYOKU: {
                            cur0 += d0, cur1 += d1, cur2 += d2, cur3 += d3;
                            const int delta = stat_pick(pid, d0, d1, d2, d3);
                            if (!seat_lane) break;
                            C[MJ_ST_RYUKYOKU] += 1;
                            C[MJ_ST_RYUKYOKU_POINT] += delta;
                            if (accepted) {
                                C[MJ_ST_RIICHI_RYUKYOKU] += 1;
                                C[MJ_ST_RIICHI_POINT] += delta - 1000;
                            } else if (fuuro > 0) {
                                C[MJ_ST_FUURO_POINT] += delta;
                            }
                            if (delta >= 8000) C[MJ_ST_NAGASHI_MANGAN] += 1;
                            break;
                        }
                        case LG_END_KYOKU:
                            if (seat_lane && fuuro > 0) {
                                C[MJ_ST_FUURO] += 1;
                                C[MJ_ST_FUURO_NUM] += fuuro;
                            }
                            break;
                        default:  // tsumo, kakan, ankan, dora
                            break;
                    }
                }
            }
            if (!bad && lane < 4) {
                // Rankings::new: stable, ties to the lower seat; the top-up to 100,000 goes to first place after ranking
                const int mine_c = stat_pick(pid, cur0, cur1, cur2, cur3);
                const int rank = (cur0 > mine_c || (cur0 == mine_c && 0 < pid)) + (cur1 > mine_c || (cur1 == mine_c && 1 < pid)) +
                                 (cur2 > mine_c || (cur2 == mine_c && 2 < pid)) + (cur3 > mine_c || (cur3 == mine_c && 3 < pid));
                const int total = cur0 + cur1 + cur2 + cur3;
                const int final_score = mine_c + (rank == 0 && total < 100000 ? 100000 - total : 0);
                C[MJ_ST_GAME] = 1;
                C[MJ_ST_POINT] = final_score - 25000;
                if (final_score < 0) C[MJ_ST_TOBI] = 1;
                C[MJ_ST_RANK_1 + rank] = 1;
            }
        }
        if (skip) n_skipped++;
        else if (bad) n_malformed++;
        else n_reduced++;
        mj_team_sync<64>();
        if (lane < MJ_STAT_FIELDS) {  // one field per lane: 44 consecutive int64 per seat row
            const bool ok = !skip && !bad;
            for (int s = 0; s < 4; s++) {
                const long long v = ok && ((seats >> s) & 1) ? s_cnt[wave][s][lane] : 0ll;
                if (P.per_seat) P.per_seat[((size_t)log * 4 + s) * MJ_STAT_FIELDS + lane] = v;
                s_tot[wave][(groups >> s) & 1][lane] += v;
            }
        }
        mj_team_sync<64>();
    }

    if (lane == 0) s_n[wave][0] = n_reduced, s_n[wave][1] = n_skipped, s_n[wave][2] = n_malformed;
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 2 * MJ_STAT_FIELDS) {
        long long sum = 0;
        for (int w = 0; w < STAT_WAVES; w++) sum += (&s_tot[w][0][0])[tid];
        if (sum) atomicAdd(&P.totals[tid], (unsigned long long)sum);
    } else if (tid < 2 * MJ_STAT_FIELDS + 3) {
        const int c = tid - 2 * MJ_STAT_FIELDS;
        unsigned long long sum = 0;
        for (int w = 0; w < STAT_WAVES; w++) sum += s_n[w][c];
        if (sum) atomicAdd(&P.counts[c], sum);
    }
}
