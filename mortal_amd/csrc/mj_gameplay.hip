// Training samples from packed event logs without a host codec (the reference's route: arena/result.rs:32-51 dump_json_log ->
// dataset/gameplay.rs:66-124 load_gz_log_files): a pool's device log becomes the replay script of another pool (mj_k_log_len,
// mj_k_log_scan, mj_k_log_pack, mj_k_log_fresh), and dataset/grp.rs:90-164 Grp::load_events is reduced from the same words
// (mj_k_log_grp).
//
// Shape: mj_log.h.  An event's length is a function of its header word alone (log_event_len), so the length pass and the copy walk
// fixed windows [64 j, 64 j + 64) and carry the chain position across them; the copy stores each window as it was loaded
// (coalesced), with LG_SK_DEAL_BIT set on the lanes the walk found to hold a start_kyoku header (a payload word can look like one:
// the headers are known only by walking).  Grp reads payload words (scores, deltas): mj_k_log_grp is a callable of log_walk_events.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mj_log.h"

// ---- suit augmentation on the way through (the reference's GameplayLoader(augmented=True): mjai/event.rs:187-217 Event::augment,
// tile.rs:154-167 Tile::augment).  What a word is -- a header, haipai tiles, wall tiles, ura indicators, or a tag / score / delta
// word that only looks like one of them -- is known from the walk alone, so the walk hands every window a few lane masks and each
// lane rewrites its own word by the mask it is in.  An event can straddle a window boundary: the walk keeps the last header it
// followed (position and both halves, wave-uniform) and enters that event's roles again in the window its payload runs into.
MJD uint32_t log_aug_tile(uint32_t t) {  // manzu <-> pinzu, 5mr <-> 5pr; ids >= 36 and the honours stay
    return t < 9 ? t + 9 : t < 18 ? t - 9 : t == 34 ? 35u : t == 35 ? 34u : t;
}
struct LogRoles {          // one bit per lane of the window
    uint64_t hdr;          // an event header: 6-bit tile fields chosen by its own type
    uint64_t bytes8;       // haipai words 1..6 and the 17 wall words: 8 tile bytes
    uint64_t bytes4;       // the 7th haipai word: tile bytes 0..3 (the upper four are unused and stay 0)
    uint64_t ura0, ura1, ura2;  // a hora's ura word: the bit planes of the header's n_ura (that many 6-bit fields from bit 0)
};
MJD uint64_t log_win_mask(uint32_t lo, uint32_t hi, uint32_t base) {  // words [lo, hi) of the log as lanes of the window at `base`
    const uint32_t a = max(lo, base), b = min(hi, base + 64u);
    if (a >= b) return 0ull;
    return (b - a == 64u ? ~0ull : (1ull << (b - a)) - 1) << (a - base);
}
// the payload roles of the event whose header (w_lo, w_hi) stands at word p, as far as they fall into the window; wave-uniform
MJD void log_roles_add(LogRoles& R, uint32_t p, uint32_t w_lo, uint32_t w_hi, uint32_t base) {
    const int t = w_lo & 15;
    if (t == LG_START_KYOKU) {
        R.bytes8 |= log_win_mask(p + 3, p + 9, base);
        R.bytes4 |= log_win_mask(p + 9, p + 10, base);
        if ((w_hi >> (LG_SK_WALL_BIT - 32)) & 1) R.bytes8 |= log_win_mask(p + 10, p + 27, base);
    } else if (t == LG_HORA) {
        const uint32_t u = p + 3 + ((w_hi >> (LG_TAG_BIT - 32)) & 1), n = (w_hi >> (LG_NURA_SHIFT - 32)) & 7;
        const uint64_t m = log_win_mask(u, u + 1, base);
        R.ura0 |= n & 1 ? m : 0ull, R.ura1 |= n & 2 ? m : 0ull, R.ura2 |= n & 4 ? m : 0ull;
    }
}
// a lane's own word through the swap; `deal`: a start_kyoku header also takes LG_SK_DEAL_BIT and LG_SK_AUG_BIT
MJD uint64_t log_aug_word(uint64_t w, const LogRoles& R, int lane, bool deal) {
    uint32_t fields = 0, width = 6, shift = 0;  // bit k of `fields`: the tile at bit shift + k * width
    if ((R.hdr >> lane) & 1) {
        const int t = (int)(w & 15);
        shift = 8;  // pai, c0, c1, c2, c3 (LG_WORD); a start_kyoku's c0 is the kyoku number, a hora header holds no tile
        fields = t == LG_START_KYOKU || t == LG_TSUMO || t == LG_DAHAI || t == LG_DORA ? 1u
                 : t == LG_CHI || t == LG_PON                                          ? 7u
                 : t == LG_DAIMINKAN || t == LG_KAKAN                                  ? 15u
                 : t == LG_ANKAN                                                       ? 30u
                                                                                       : 0u;
        if (deal && t == LG_START_KYOKU) w |= (1ull << LG_SK_DEAL_BIT) | (1ull << LG_SK_AUG_BIT);
    } else if ((R.bytes8 >> lane) & 1) {
        fields = 0xFFu, width = 8;
    } else if ((R.bytes4 >> lane) & 1) {
        fields = 0x0Fu, width = 8;
    } else {
        const uint32_t n = (uint32_t)((R.ura0 >> lane) & 1) | (uint32_t)((R.ura1 >> lane) & 1) << 1 | (uint32_t)((R.ura2 >> lane) & 1) << 2;
        fields = (1u << n) - 1;
    }
    const uint64_t in = w;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t sh = shift + k * width, t = (uint32_t)(in >> sh) & ((1u << width) - 1);
        if ((fields >> k) & 1) w ^= (uint64_t)(t ^ log_aug_tile(t)) << sh;
    }
    return w;
}

// Walks the chain of one log in fixed 64-word windows (it reads no payload, so unlike log_walk_events it never restarts one).  `store`: NULL, or where the words go; `deal_bit`: set LG_SK_DEAL_BIT in
// every start_kyoku header on the way.  -> the chain is a sequence of known events that ends exactly at `len`.
// AUG: the stored words are suit-augmented (above), and `deal_bit` sets LG_SK_AUG_BIT as well; the plain walk is what it was.
template <bool AUG>
MJD bool log_walk(const uint64_t* lw, uint32_t len, int lane, uint64_t* store, bool deal_bit) {
    uint32_t pos = 0;  // wave-uniform: the next header
    bool bad = false;
    uint32_t ev_pos = 0, ev_lo = 0, ev_hi = 0;  // AUG, wave-uniform: the last header followed
    for (uint32_t base = 0; base < len; base += 64) {
        const uint64_t mine = base + (uint32_t)lane < len ? lw[base + lane] : 0ull;  // never beyond len
        const uint32_t end = min(base + 64u, len);
        uint64_t sk = 0;  // window lanes that hold a start_kyoku header
        LogRoles R{};
        if constexpr (AUG)
            if (pos > base) log_roles_add(R, ev_pos, ev_lo, ev_hi, base);  // the payload the previous window left behind
        while (pos < end && !bad) {
            const int k = __builtin_amdgcn_readfirstlane((int)(pos - base));
            uint32_t w_lo, w_hi;
            if (!log_header(mine, k, w_lo, w_hi)) bad = true;
            if ((w_lo & 15) == LG_START_KYOKU) sk |= 1ull << k;
            if constexpr (AUG) {
                R.hdr |= 1ull << k;
                log_roles_add(R, pos, w_lo, w_hi, base);
                ev_pos = pos, ev_lo = w_lo, ev_hi = w_hi;
            }
            pos += (uint32_t)log_event_len(w_lo, w_hi);
        }
        if constexpr (AUG) {
            if (store && base + (uint32_t)lane < len) store[base + lane] = log_aug_word(mine, R, lane, deal_bit);
        } else {
            if (store && base + (uint32_t)lane < len)
                store[base + lane] = mine | (deal_bit && ((sk >> lane) & 1) ? 1ull << LG_SK_DEAL_BIT : 0ull);
        }
        if (bad && !store) break;
    }
    return !bad && pos == len;
}

// ---- pass 1: per log the number of words its script takes (0: skipped or malformed), and the three counts
struct LogLenParams {
    LogSrc src;
    uint32_t* len_out;           // [n_logs]
    unsigned long long* counts;  // [3] loaded / skipped / malformed, added to
};
__global__ __launch_bounds__(LOG_THREADS) void mj_k_log_len(LogLenParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LogCounts n;
    for (int i = blockIdx.x * LOG_WAVES + wave; i < P.src.n_logs; i += gridDim.x * LOG_WAVES) {
        const uint64_t* lw;
        uint32_t len;
        int st = log_locate(P.src, i, lw, len);
        if (st == LOG_OK && !log_walk<false>(lw, len, lane, nullptr, false)) st = LOG_BAD;
        if (lane == 0) P.len_out[i] = st == LOG_OK ? len : 0u;
        n.add(st);
    }
    n.flush(lane, P.counts);
}

// ---- pass 2: exclusive scan of the lengths, one workgroup; off[n] = the total's low word, *total = the total
__global__ __launch_bounds__(1024) void mj_k_log_scan(const uint32_t* len, int n, uint32_t* off, unsigned long long* total) {
    __shared__ unsigned long long s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const unsigned long long v = i < n ? len[i] : 0u;
        unsigned long long x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        unsigned long long before = 0, tile = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) before += s_wave[w];
            tile += s_wave[w];
        }
        if (i < n) off[i] = (uint32_t)(carry + before + x - v);
        carry += tile;
        __syncthreads();
    }
    if (tid == 0) {
        off[n] = (uint32_t)carry;
        *total = carry;
    }
}

// ---- pass 3: the copy.  Log i goes to script[off[i] .. off[i + 1]) (an empty range for a skipped or malformed one).
struct LogPackParams {
    LogSrc src;
    const uint32_t* off;  // [n_logs + 1]
    uint64_t* script;
    int deal_from_seed;
};
// AUG: the words go through the suit swap (log_walk<true>); the plain instantiation is the copy it was

template <bool AUG>
__global__ __launch_bounds__(LOG_THREADS) void mj_k_log_pack(LogPackParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * LOG_WAVES + wave; i < P.src.n_logs; i += gridDim.x * LOG_WAVES) {
        const uint32_t n = P.off[i + 1] - P.off[i];
        if (n == 0) continue;
        const uint64_t* lw;
        uint32_t len;
        log_locate(P.src, i, lw, len);  // (n == len: pass 1 accepted this log)
        uint64_t* out = P.script + (size_t)P.off[i];
        if constexpr (AUG) {
            log_walk<true>(lw, n, lane, out, P.deal_from_seed != 0);
        } else if (P.deal_from_seed) {
            log_walk<false>(lw, n, lane, out, true);
        } else {
            for (uint32_t k = lane; k < n; k += 64) out[k] = lw[k];
        }
    }
}

// ---- the destination's tables at the start of a replay (mj_capi.hip fresh_blocks, on the device): `fresh` arrives zeroed; the
// padding lanes of the last block are inactive; with `src`, table i takes the seed of the source's table table0 + i; with plain
// `nonces` / `keys` arrays (a harvest's records), table i takes nonces[i], keys[i]
__global__ __launch_bounds__(64) void mj_k_log_fresh(TableBlock* fresh, int n_tables, const TableBlock* src, int table0,
                                                     const uint64_t* nonces, const uint64_t* keys) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    TableBlock* B = fresh + blockIdx.x;
    const int l = threadIdx.x;
    if (i >= n_tables) {
        B->flags[l] = TF_INACTIVE | TF_DONE | TF_ENDED;
    } else if (src) {
        const int t = table0 + i;
        B->seed_nonce[l] = src[t >> 6].seed_nonce[t & 63];
        B->seed_key[l] = src[t >> 6].seed_key[t & 63];
    } else if (nonces) {
        B->seed_nonce[l] = nonces[i];
        B->seed_key[l] = keys[i];
    }
}

// ---- Grp::load_events (dataset/grp.rs:90-164), forwards: a start_kyoku records its row and restarts the running scores, hora /
// ryukyoku add their deltas, reach_accepted takes 1000; what stands at the end is what the reference's reverse walk collects up
// to the last start_kyoku.
struct GrpParams {
    LogSrc src;
    int max_kyoku;
    int32_t* feat;      // [n_logs][max_kyoku][7] raw: grand kyoku, honba, kyotaku, scores[4]; zeroed by the caller
    int32_t* n_kyoku;   // [n_logs]: rows written; 0 for a skipped log, -1 for a malformed one
    int32_t* rank;      // [n_logs][4] rank_by_player
    int32_t* final_;    // [n_logs][4] final_scores
    unsigned long long* counts;  // [3] reduced / skipped / malformed, added to
};
__global__ __launch_bounds__(LOG_THREADS) void mj_k_log_grp(GrpParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LogCounts n;
    for (int log = blockIdx.x * LOG_WAVES + wave; log < P.src.n_logs; log += gridDim.x * LOG_WAVES) {
        const uint64_t* lw;
        uint32_t len;
        int st = log_locate(P.src, log, lw, len);
        int32_t* const F = P.feat + (size_t)log * P.max_kyoku * 7;
        int nk = 0;  // wave-uniform
        LogScores sc;
        if (st == LOG_OK) {
            const bool ok = log_walk_events(lw, len, lane, sc, [&](const LogEvent& e) {
                if (e.type != LG_START_KYOKU) return true;
                if (nk >= P.max_kyoku) return false;
                const int c0 = (e.w_lo >> 14) & 63;  // bakaze * 4 + kyoku - 1; grp.rs:135-139 counts west and north alike
                const int grand = c0 < 12 ? c0 : c0 - 4;
                const int honba = (e.w_hi >> (LG_HONBA_SHIFT - 32)) & 0xFF, kyotaku = (e.w_hi >> (LG_KYOTAKU_SHIFT - 32)) & 0xFF;
                if (lane < 7)
                    F[nk * 7 + lane] = lane == 0 ? grand : lane == 1 ? honba : lane == 2 ? kyotaku : log_pick(lane - 3, e.d0, e.d1, e.d2, e.d3);
                nk++;
                return true;
            });
            if (!ok || nk == 0) {
                st = LOG_BAD;
                for (int r = 0; r < nk; r++)  // (the lanes that wrote the rows take them back)
                    if (lane < 7) F[r * 7 + lane] = 0;
            }
        }
        if (lane < 4) {
            int rank = 0, final_score = 0;
            if (st == LOG_OK) sc.final_of(lane, rank, final_score);
            P.rank[(size_t)log * 4 + lane] = rank;
            P.final_[(size_t)log * 4 + lane] = final_score;
        }
        if (lane == 0) P.n_kyoku[log] = st == LOG_OK ? nk : st == LOG_SKIP ? 0 : -1;
        n.add(st);
    }
    n.flush(lane, P.counts);
}
