// Sample store (include/mortal_amd.h mj_samples_*): a replayed decision kept as what the encoders read of it -- its snapshot record
// and a row descriptor -- plus the eight int32 of mj_k_replay_meta, instead of its obs.  mj_k_encode<V>, mj_k_sp* and
// mj_k_encode_oracle address a row as snap + ROW_TABLE(desc) and nothing else, so a list of store indices turned into descriptors
// (mj_k_samples_rows) is encoded in place on the store's record array by the unchanged kernels.
// Reference counterpart: the buffer of mortal/dataloader.py (populate_buffer keeps every obs of a file batch, then shuffles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mj_state.h"

static_assert(sizeof(TableOne) % 64 == 0, "a record is copied as whole 16-byte pieces, four to a 64-byte line");

struct SamplesAppendParams {
    const TableOne* snap;      // the replay pool's snapshot records
    const TableBlock* blocks;  // ... and its tables (at_turn, shanten: where mj_k_replay_meta reads them)
    const uint32_t* rows;      // agent 0's row descriptors of the current batch
    int n_rows;
    const int32_t* label;
    const int32_t* kan_label;
    const uint8_t* kyoku_idx;
    const uint32_t* ev_index;
    int32_t log_base;  // game number of the pool's table 0
    TableOne* rec;     // the store's arrays, from its first free sample on
    uint32_t* desc;
    int32_t* meta;     // [n_rows][8]
};

// One wavefront per row: the record in 16-byte pieces (rows of one step that name the same table each get their own copy), the
// descriptor without its table, the meta of mj_k_replay_meta with the game number in place of the table.
__global__ __launch_bounds__(64) void mj_k_samples_append(SamplesAppendParams P) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= P.n_rows) return;
    const uint32_t d = P.rows[r];
    const int t = ROW_TABLE(d), s = ROW_SEAT(d), kan = ROW_KAN(d);
    const float4* src = reinterpret_cast<const float4*>(P.snap + t);
    float4* dst = reinterpret_cast<float4*>(P.rec + r);
    // whole rounds of the 64 lanes two at a time (named registers: an indexed array of them is lowered to LDS), then the lanes the
    // last pieces need; a pair's loads are both issued before its first store
    constexpr int PIECES = (int)(sizeof(TableOne) / 16), FULL = PIECES / 64, TAIL = PIECES % 64;
    float4 last = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < TAIL) last = src[lane + 64 * FULL];
#pragma unroll
    for (int k = 0; k < FULL; k += 2) {
        const float4 a = src[lane + 64 * k];
        const float4 b = k + 1 < FULL ? src[lane + 64 * (k + 1)] : a;
        dst[lane + 64 * k] = a;
        if (k + 1 < FULL) dst[lane + 64 * (k + 1)] = b;
    }
    if (lane < TAIL) dst[lane + 64 * FULL] = last;
    if (lane == 0) P.desc[r] = ROW_PACK(0, s, kan);
    if (lane < 8) {
        const TableBlock* B = P.blocks + (t >> 6);
        const int l = t & 63;
        int32_t v;
        switch (lane) {
            case 0: v = kan ? P.kan_label[t * 4 + s] : P.label[t * 4 + s]; break;
            case 1: v = P.log_base + t; break;
            case 2: v = s; break;
            case 3: v = P.kyoku_idx[t]; break;
            case 4: v = B->at_turn[s][l]; break;
            case 5: v = B->shanten[s][l]; break;
            case 6: v = kan; break;
            default: v = (int32_t)P.ev_index[t]; break;
        }
        P.meta[(size_t)r * 8 + lane] = v;
    }
}

// One thread per requested sample: its index is the "table" of the row the encoders get.  The host has range-checked idx.
__global__ __launch_bounds__(256) void mj_k_samples_rows(const int32_t* idx, const uint32_t* desc, int n, uint32_t* rows_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = (uint32_t)idx[i];
    rows_out[i] = k | desc[k];
}
