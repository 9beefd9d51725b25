// gol_settle.h -- K1r2s k_settle_resident_batch: k_step_resident_batch's turn with a watch on every
// board that finds the board's period exactly and skips the turns of a board known to repeat
// (gol_settle.hip holds the kernel, its launch and the library's device-free model of it;
// gol_batch.cpp the gol_settle_* calls).
//
// The watch of a board that started at turn `start` keeps a snapshot of it, taken at turns
// s_k = start + 2^k - 1 (Brent's schedule).  The board after every watched turn t is compared
// with the snapshot, every word of every real row; at t == s_k + 2^k the compare comes first and
// a board that does not match becomes snapshot k + 1.  The first match gives period = t - s_k
// (the minimal period of the cycle) and settled_turn = t.  From then on an advance of d turns
// runs d mod period turns.
//
// The state of a board lives in device memory beside the boards: its SettleState and its
// snapshot (height x nw words, the board's layout).  A workgroup reads both at launch start and
// writes back what it changed.  The snapshot sits in registers like the board.  A lane's compare
// result joins the turn's one barrier: the wave reduces it, one lane per wave leaves it in the
// LDS word [turn parity][wave], and after the barrier every wave reads all the words, so the
// match, the re-snapshot and the exit from the watched loop are workgroup-uniform.  The words are
// double-buffered by parity for xch's reason (gol_resident.h): a wave that writes the word of
// turn t + 2 has passed barrier t + 1, which every wave reaches after its reads of turn t.
#pragma once
#include "gol_resident.h"

namespace golk {

constexpr int kSettleMaxDepth = 256;       // turns per launch (GOL_SETTLE_DEPTH chooses 1 .. this)
constexpr int kSettleWaves = kResidentMaxLanes / 64;

struct SettleState {
    long long start;                       // the turn the watch began at
    long long k;                           // the snapshot held is number k, taken at s_k
    long long period;                      // 0 = unknown
    long long settled_turn;                // -1 = unknown
};

// s_k: the turn snapshot k of a watch from `start` is taken at
__host__ __device__ inline long long settle_snap_turn(long long start, long long k)
{
    return start + (1ll << k) - 1;
}
// the LDS word of a wave's compare result: [turn parity][wave]
__host__ __device__ constexpr int settle_flag_words() { return 2 * kSettleWaves; }
__host__ __device__ inline int settle_flag_index(int parity, int wave) { return parity * kSettleWaves + wave; }
// turns a board of known period runs for an advance of `turns` (1 .. kSettleMaxDepth) turns
__host__ __device__ inline int settle_skip_turns(long long turns, long long period)
{
    return period > turns ? (int)turns : (int)turns % (int)period;
}
// the depth of the next launch of a step with `left` turns to go: ceil(left / depth) launches of
// near-equal depth (gol_batch_step's split)
__host__ __device__ inline int settle_next_depth(long long left, int depth)
{
    const long long nl = (left + depth - 1) / depth;
    return (int)((left + nl - 1) / nl);
}

// what differs between a lane's real rows and the snapshot of them: the OR of v ^ snap (rows past
// `mine` hold garbage and take no part; a lane past the board has none: 0)
template <int NW, int R, bool RAG>
__host__ __device__ __forceinline__ uint64_t settle_diff(const uint64_t (&v)[R][NW],
                                                         const uint64_t (&snap)[R][NW], int mine)
{
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const uint64_t x = v[i][j] ^ snap[i][j];
            d |= (RAG ? i < mine : mine > 0) ? x : 0ull;
        }
    return d;
}

}  // namespace golk
