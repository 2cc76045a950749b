// libriichi's Stat on the device: mj_k_log_stat reduces packed event logs (mj_state.h LG_* words) to the 44 counters of
// `Stat` (stat.rs:30-126), event by event as Stat::from_game does (stat.rs:263-441; host reading: mortal_amd/stat.py).
// Field order: include/mortal_amd.h MjStatField.
//
// Shape: mj_log.h -- one wavefront per log, the chain followed by log_walk_events; this file is what Stat does with an event.  The
// event and the scores are wave-uniform; lanes 0..3 each follow one seat (jun, fuuro count, riichi declared / accepted, others'
// riichi) and own that seat's 44 counters in LDS.  A finished log is handed to lanes 0..43 (one field each) that store the
// per-seat rows and add the selected seats to the wavefront's totals; the workgroup's four wavefronts are summed once at the end,
// one 64-bit atomicAdd per non-zero field (and count) and workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mortal_amd.h"
#include "mj_log.h"

struct StatParams {
    LogSrc src;
    const uint8_t* seats;        // [n_logs] 4-bit seat masks, NULL = all four
    const uint8_t* groups;       // [n_logs] bit s = group of seat s, NULL = 0 (pool path: agent_of_seat of the table instead)
    unsigned long long* totals;  // [2][MJ_STAT_FIELDS], added to
    long long* per_seat;         // NULL or [n_logs][4][MJ_STAT_FIELDS], every row written
    unsigned long long* counts;  // [3] logs reduced / skipped / malformed, added to
};

__global__ __launch_bounds__(LOG_THREADS) void mj_k_log_stat(StatParams P) {
    __shared__ long long s_cnt[LOG_WAVES][4][MJ_STAT_FIELDS];            // the current log's counters, per seat
    __shared__ long long s_tot[LOG_WAVES][2][MJ_STAT_FIELDS];            // the wavefront's totals, per group
    __shared__ unsigned s_n[LOG_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pid = lane & 3;  // (lanes >= 4 follow the walk for the collectives only)
    long long* const C = &s_cnt[wave][pid][0];
    long long* const flat = &s_cnt[wave][0][0];
    for (int i = lane; i < 2 * MJ_STAT_FIELDS; i += 64) (&s_tot[wave][0][0])[i] = 0;
    LogCounts n;

    for (int log = blockIdx.x * LOG_WAVES + wave; log < P.src.n_logs; log += gridDim.x * LOG_WAVES) {
        const uint64_t* lw;
        uint32_t len;
        int st = log_locate(P.src, log, lw, len);
        const uint32_t seats = P.seats ? P.seats[log] & 15u : 15u;
        uint32_t groups = P.groups ? P.groups[log] : 0u;
        if (P.src.blocks) {
            const int t = P.src.table0 + log;
            groups = P.src.blocks[t >> 6].agent_of_seat[t & 63];
        }
        for (int i = lane; i < 4 * MJ_STAT_FIELDS; i += 64) flat[i] = 0;
        mj_team_sync<64>();

        if (st == LOG_OK) {
            LogScores sc;
            int oya = 0;                                                            // wave-uniform
            bool declared = false, accepted = false, others_declared = false;       // this lane's seat
            int jun = 0, fuuro = 0;
            const bool seat_lane = lane < 4;
            const bool ok = log_walk_events(lw, len, lane, sc, [&](const LogEvent& e) {
                const int actor = e.actor, target = e.target;
                const bool me = actor == pid;
                const bool is_oya = oya == pid;
                switch (e.type) {
                    case LG_START_KYOKU:
                        oya = (int)((e.w_lo >> 14) & 63) & 3;  // kyoku % 4 (the kyoku index 0..15 travels in c0)
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
                        if (me) accepted = true;
                        break;
                    case LG_HORA: {
                        const int delta = log_pick(pid, e.d0, e.d1, e.d2, e.d3);
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
                        const int delta = log_pick(pid, e.d0, e.d1, e.d2, e.d3);
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
                return true;  // (Stat refuses nothing the chain allows)
            });
            if (!ok) st = LOG_BAD;
            if (ok && lane < 4) {
                int rank, final_score;
                sc.final_of(pid, rank, final_score);
                C[MJ_ST_GAME] = 1;
                C[MJ_ST_POINT] = final_score - 25000;
                if (final_score < 0) C[MJ_ST_TOBI] = 1;
                C[MJ_ST_RANK_1 + rank] = 1;
            }
        }
        n.add(st);
        mj_team_sync<64>();
        if (lane < MJ_STAT_FIELDS) {  // one field per lane: 44 consecutive int64 per seat row
            for (int s = 0; s < 4; s++) {
                const long long v = st == LOG_OK && ((seats >> s) & 1) ? s_cnt[wave][s][lane] : 0ll;
                if (P.per_seat) P.per_seat[((size_t)log * 4 + s) * MJ_STAT_FIELDS + lane] = v;
                s_tot[wave][(groups >> s) & 1][lane] += v;
            }
        }
        mj_team_sync<64>();
    }

    if (lane < 3) s_n[wave][lane] = n.of_lane(lane);  // (not LogCounts::flush: summed per workgroup first)
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 2 * MJ_STAT_FIELDS) {
        long long sum = 0;
        for (int w = 0; w < LOG_WAVES; w++) sum += (&s_tot[w][0][0])[tid];
        if (sum) atomicAdd(&P.totals[tid], (unsigned long long)sum);
    } else if (tid < 2 * MJ_STAT_FIELDS + 3) {
        const int c = tid - 2 * MJ_STAT_FIELDS;
        unsigned long long sum = 0;
        for (int w = 0; w < LOG_WAVES; w++) sum += s_n[w][c];
        if (sum) atomicAdd(&P.counts[c], sum);
    }
}
