// gol_settle.hip -- K1r2s k_settle_resident_batch (gol_settle.h): the kernel, its instantiation
// table and launch, k_settle_init, and the device-free export gol_settle_host_run.
#include "gol_settle.h"

#include <cstdint>
#include <type_traits>
#include <vector>

#include "gol_amd.h"
#include "gol_kernels.h"

namespace golk {

namespace {

// Workgroup b advances board b of a batch (k_step_resident_batch's layout, IN PLACE) from turn
// `turn0` by `turns` turns (1 .. kSettleMaxDepth), under the watch states[b] with its snapshot at
// snaps + b x height x NW.  All of these are uniform: kernel arguments, or read from states[b]
// by every lane alike, or read from the LDS words `flag` after a barrier by every wave alike.
//
// A board of known period runs settle_skip_turns(turns, period) plain turns and nothing else.
// A watched board runs the loop below: iteration t holds the board at turn T = turn0 + t.
//   - it publishes its first and last row as k_step_resident_batch does; where T is past the
//     snapshot's turn it also compares (settle_diff), the wave reduces by ballot, and lane 0 of
//     the wave writes the wave's word of parity t & 1;
//   - the turn's one barrier;
//   - north and south, and every wave reads all the waves' words in one 16-byte read (issued
//     together: one LDS latency).  All equal: the match -- period = T - s_k, settled_turn = T,
//     and the loop ends; the rest of the launch is (turn0 + turns - T) mod period plain turns;
//   - no match and T == s_k + 2^k: the board becomes snapshot k + 1;
//   - resident_turn.
// After the last turn the board is compared once more, behind a barrier of its own, so a launch
// of a watched board has turns + 1 barriers and results do not depend on where launches end.
// Every launched wave runs every iteration and reaches every barrier: the exits depend on
// uniform values only.
// At the end the lanes store the board's rows, the snapshot's rows if it changed, and lane 0
// the state if it changed.
template <int NW, int R>
__global__ __launch_bounds__(kResidentMaxLanes) void k_settle_resident_batch(
    uint64_t *words, uint64_t *snaps, SettleState *states, int width, int height, long long turn0,
    int turns)
{
    __shared__ uint64_t xch[resident_xch_words(NW)];
    __shared__ __attribute__((aligned(16))) uint32_t flag[settle_flag_words()];
    const size_t base = (size_t)blockIdx.x * (size_t)height * (size_t)NW;
    uint64_t *board = words + base;
    uint64_t *snapb = snaps + base;
    SettleState st = states[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int lanes = (height + R - 1) / R;
    const bool active = lane < lanes;
    const int mine = resident_rows_of(lane, R, height);
    const int nb = resident_tail_bits(width, NW);
    const uint64_t tail = resident_tail_mask(nb);
    const int ln = active ? resident_north_lane(lane, lanes) : 0;
    const int ls = active ? resident_south_lane(lane, lanes) : 0;
    const size_t row0 = (size_t)lane * R;
    const int nwaves = (int)blockDim.x >> 6;

    // (the words of waves that are not launched: 0, before the first barrier)
    if (lane < settle_flag_words() && lane % kSettleWaves >= nwaves) flag[lane] = 0;

    uint64_t v[R][NW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) v[i][j] = i < mine ? board[(row0 + i) * (size_t)NW + j] : 0ull;

    auto run = [&](auto rag) {
        constexpr bool RAG = decltype(rag)::value;
        // n plain turns (k_step_resident_batch's), the first on parity p0
        auto plain = [&](int p0, int n) {
            for (int t = 0; t < n; ++t) {
                const int p = (p0 + t) & 1;
                if (active) {
                    uint64_t last[NW];
                    resident_last_row<NW, R, RAG>(v, mine, last);
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        xch[resident_xch_index(NW, p, 0, j, lane)] = v[0][j];
                        xch[resident_xch_index(NW, p, 1, j, lane)] = last[j];
                    }
                }
                __syncthreads();
                uint64_t north[NW], south[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    north[j] = xch[resident_xch_index(NW, p, 1, j, ln)];
                    south[j] = xch[resident_xch_index(NW, p, 0, j, ls)];
                }
                resident_turn<NW, R, RAG>(v, north, south, mine, nb, tail);
            }
        };
        if (st.period != 0) {
            plain(0, settle_skip_turns(turns, st.period));
            return;
        }

        uint64_t snap[R][NW];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int j = 0; j < NW; ++j)
                snap[i][j] = i < mine ? snapb[(row0 + i) * (size_t)NW + j] : 0ull;
        long long snap_turn = settle_snap_turn(st.start, st.k);
        long long span = 1ll << st.k;
        bool snapped = false;
        // before a barrier: the wave's compare of the board with the snapshot into its word
        auto vote = [&](int p) {
            const uint64_t d = settle_diff<NW, R, RAG>(v, snap, mine);
            const bool differs = __builtin_amdgcn_ballot_w64(d != 0) != 0;
            if ((lane & 63) == 0) flag[settle_flag_index(p, lane >> 6)] = differs ? 1u : 0u;
        };
        // after it: every wave's word in one read (a wave that is not launched: 0); all equal?
        auto agreed = [&](int p) {
            const uint4 f = *reinterpret_cast<const uint4 *>(&flag[settle_flag_index(p, 0)]);
            return __builtin_amdgcn_readfirstlane((int)(f.x | f.y | f.z | f.w)) == 0;
        };
        auto matched = [&](long long T) {
            st.period = T - snap_turn;
            st.settled_turn = T;
        };
        // no match at the snapshot's last turn: the board is the next snapshot
        auto resnap = [&](long long T) {
            if (T != snap_turn + span) return;
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < NW; ++j) snap[i][j] = v[i][j];
            snap_turn = T;
            span *= 2;
            st.k += 1;
            snapped = true;
        };
        // iteration t up to the agreement: publish, vote, the barrier, north and south, all equal?
        uint64_t north[NW], south[NW];
        auto look = [&](int t) {
            const int p = t & 1;
            if (active) {
                uint64_t last[NW];
                resident_last_row<NW, R, RAG>(v, mine, last);
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    xch[resident_xch_index(NW, p, 0, j, lane)] = v[0][j];
                    xch[resident_xch_index(NW, p, 1, j, lane)] = last[j];
                }
            }
            vote(p);
            __syncthreads();
            uint4 f = *reinterpret_cast<const uint4 *>(&flag[settle_flag_index(p, 0)]);
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                north[j] = xch[resident_xch_index(NW, p, 1, j, ln)];
                south[j] = xch[resident_xch_index(NW, p, 0, j, ls)];
            }
            // (the three reads are in flight together: left alone, the compiler sinks north and
            // south below the branch on the words, a second LDS latency in every turn)
#pragma unroll
            for (int j = 0; j < NW; ++j) asm volatile("" : "+v"(north[j]), "+v"(south[j]), "+v"(f.x));
            return __builtin_amdgcn_readfirstlane((int)(f.x | f.y | f.z | f.w)) == 0;
        };
        // The iterations are cut where the snapshot changes, so the loop that runs most turns
        // holds one snapshot and has one exit test.  (Only iteration 0 can hold the board at the
        // snapshot's own turn -- a fresh watch, or a launch that begins where the last one
        // re-snapshot: a plain turn, nothing to compare.)
        int t = 0;
        bool match = false;
        if (turn0 == snap_turn) {
            plain(0, 1);
            t = 1;
        }
        for (;;) {
            const long long left = snap_turn + span - turn0;         // iteration of the re-snapshot
            const int tsnap = left > turns ? turns : (int)left;
            for (; t < tsnap; ++t) {
                if ((match = look(t))) break;
                resident_turn<NW, R, RAG>(v, north, south, mine, nb, tail);
            }
            if (match || t >= turns) break;
            // T == s_k + 2^k: the compare comes first, then the board becomes snapshot k + 1
            if ((match = look(t))) break;
            resnap(turn0 + t);
            resident_turn<NW, R, RAG>(v, north, south, mine, nb, tail);
            ++t;
        }
        if (match) {
            matched(turn0 + t);
        } else {
            // the board after the launch's last turn (past the snapshot's turn: turns >= 1)
            const long long T = turn0 + turns;
            vote(turns & 1);
            __syncthreads();
            if (agreed(turns & 1)) matched(T);
            else resnap(T);
        }
        if (st.period != 0) {
            // (the rows published in iteration t were not read: the next parity is free)
            plain((t + 1) & 1, settle_skip_turns(turn0 + turns - st.settled_turn, st.period));
        } else if (snapped) {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (i < mine) snapb[(row0 + i) * (size_t)NW + j] = snap[i][j];
        }
        if (lane == 0 && (st.period != 0 || snapped)) states[blockIdx.x] = st;
    };
    // (uniform: only the board's last lane can own fewer than R rows)
    if (R > 1 && height % R != 0) run(std::true_type{});
    else run(std::false_type{});

#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j)
            if (i < mine) board[(row0 + i) * (size_t)NW + j] = v[i][j];
}

// the watch of boards first .. first + n - 1 begins at `turn` (their snapshot 0 is copied by the
// caller)
__global__ __launch_bounds__(256) void k_settle_init(SettleState *states, int first, int n,
                                                     long long turn)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) states[first + i] = SettleState{turn, 0, 0, -1};
}

void *settle_kernel(int nw, int R)
{
#define GOL_SETTLE_CASE(NW, R) \
    case NW * 100 + R: return reinterpret_cast<void *>(&k_settle_resident_batch<NW, R>)
    switch (nw * 100 + R) {
    GOL_SETTLE_CASE(1, 1);
    GOL_SETTLE_CASE(1, 2);
    GOL_SETTLE_CASE(1, 4);
    GOL_SETTLE_CASE(1, 8);
    GOL_SETTLE_CASE(1, 16);
    GOL_SETTLE_CASE(2, 1);
    GOL_SETTLE_CASE(2, 2);
    GOL_SETTLE_CASE(2, 4);
    GOL_SETTLE_CASE(2, 8);
    GOL_SETTLE_CASE(3, 1);
    GOL_SETTLE_CASE(3, 2);
    GOL_SETTLE_CASE(3, 4);
    GOL_SETTLE_CASE(3, 5);
    GOL_SETTLE_CASE(4, 1);
    GOL_SETTLE_CASE(4, 2);
    GOL_SETTLE_CASE(4, 4);
    default: return nullptr;
    }
#undef GOL_SETTLE_CASE
}

// The host build of the kernel for one (NW, R) and one board: the same functions lane by lane,
// arrays for the exchange area and the waves' words, and the board, the snapshot and the state
// kept in "device memory" between launches and reloaded by each.
template <int NW, int R>
struct HostSettle {
    struct Regs {
        uint64_t v[R][NW];
    };
    int width, height, lanes, nb, nwaves;
    uint64_t tail;
    bool rag;
    std::vector<uint64_t> words, snaps;      // device memory: the board, its snapshot
    SettleState state{0, 0, 0, -1};
    std::vector<uint64_t> xch = std::vector<uint64_t>((size_t)resident_xch_words(NW), 0);
    uint32_t flag[settle_flag_words()] = {};

    HostSettle(const uint64_t *in, int w, int h)
        : width(w), height(h), lanes((h + R - 1) / R), nb(resident_tail_bits(w, NW)),
          nwaves((lanes + 63) / 64), tail(resident_tail_mask(nb)), rag(R > 1 && h % R != 0),
          words(in, in + (size_t)h * NW), snaps(in, in + (size_t)h * NW)
    {
    }
    int mine(int lane) const { return resident_rows_of(lane, R, height); }
    void load(const std::vector<uint64_t> &mem, std::vector<Regs> &regs) const
    {
        for (int lane = 0; lane < lanes; ++lane)
            for (int i = 0; i < mine(lane); ++i)
                for (int j = 0; j < NW; ++j) regs[lane].v[i][j] = mem[((size_t)lane * R + i) * NW + j];
    }
    void store(const std::vector<Regs> &regs, std::vector<uint64_t> &mem) const
    {
        for (int lane = 0; lane < lanes; ++lane)
            for (int i = 0; i < mine(lane); ++i)
                for (int j = 0; j < NW; ++j) mem[((size_t)lane * R + i) * NW + j] = regs[lane].v[i][j];
    }
    void publish(const std::vector<Regs> &regs, int p)
    {
        for (int lane = 0; lane < lanes; ++lane) {
            const uint64_t (&v)[R][NW] = regs[lane].v;
            uint64_t last[NW];
            if (rag) resident_last_row<NW, R, true>(v, mine(lane), last);
            else resident_last_row<NW, R, false>(v, mine(lane), last);
            for (int j = 0; j < NW; ++j) {
                xch[resident_xch_index(NW, p, 0, j, lane)] = v[0][j];
                xch[resident_xch_index(NW, p, 1, j, lane)] = last[j];
            }
        }
    }
    void turn(std::vector<Regs> &regs, int p)
    {
        for (int lane = 0; lane < lanes; ++lane) {
            uint64_t (&v)[R][NW] = regs[lane].v;
            uint64_t north[NW], south[NW];
            for (int j = 0; j < NW; ++j) {
                north[j] = xch[resident_xch_index(NW, p, 1, j, resident_north_lane(lane, lanes))];
                south[j] = xch[resident_xch_index(NW, p, 0, j, resident_south_lane(lane, lanes))];
            }
            if (rag) resident_turn<NW, R, true>(v, north, south, mine(lane), nb, tail);
            else resident_turn<NW, R, false>(v, north, south, mine(lane), nb, tail);
        }
    }
    void plain(std::vector<Regs> &regs, int p0, int n)
    {
        for (int t = 0; t < n; ++t) {
            publish(regs, (p0 + t) & 1);
            // (the workgroup barrier)
            turn(regs, (p0 + t) & 1);
        }
    }
    // one launch: the kernel's body
    void launch(long long turn0, int turns)
    {
        SettleState st = state;
        std::vector<Regs> v((size_t)lanes, Regs{}), snap((size_t)lanes, Regs{});
        load(words, v);
        if (st.period != 0) {
            plain(v, 0, settle_skip_turns(turns, st.period));
            store(v, words);
            return;
        }
        load(snaps, snap);
        long long snap_turn = settle_snap_turn(st.start, st.k);
        long long span = 1ll << st.k;
        bool snapped = false;
        auto vote = [&](int p) {
            for (int w = 0; w < nwaves; ++w) {
                bool differs = false;                        // (the wave's ballot)
                for (int lane = 64 * w; lane < 64 * (w + 1); ++lane) {
                    // (lanes past the board hold zero rows and own none)
                    const Regs zero{};
                    const Regs &a = lane < lanes ? v[lane] : zero;
                    const Regs &b = lane < lanes ? snap[lane] : zero;
                    const int m = lane < lanes ? mine(lane) : 0;
                    const uint64_t d = rag ? settle_diff<NW, R, true>(a.v, b.v, m)
                                           : settle_diff<NW, R, false>(a.v, b.v, m);
                    differs = differs || d != 0;
                }
                flag[settle_flag_index(p, w)] = differs ? 1u : 0u;
            }
        };
        auto agreed = [&](int p) {                           // (all four words: the rest are 0)
            uint32_t f = 0;
            for (int w = 0; w < kSettleWaves; ++w) f |= flag[settle_flag_index(p, w)];
            return f == 0;
        };
        auto matched = [&](long long T) {
            st.period = T - snap_turn;
            st.settled_turn = T;
        };
        auto resnap = [&](long long T) {
            if (T != snap_turn + span) return;
            snap = v;
            snap_turn = T;
            span *= 2;
            st.k += 1;
            snapped = true;
        };
        for (int w = nwaves; w < kSettleWaves; ++w)          // (waves that are not launched)
            flag[settle_flag_index(0, w)] = flag[settle_flag_index(1, w)] = 0;
        auto look = [&](int t) {
            publish(v, t & 1);
            vote(t & 1);
            // (the workgroup barrier)
            return agreed(t & 1);
        };
        int t = 0;
        bool match = false;
        if (turn0 == snap_turn) {
            plain(v, 0, 1);
            t = 1;
        }
        for (;;) {
            const long long left = snap_turn + span - turn0;
            const int tsnap = left > turns ? turns : (int)left;
            for (; t < tsnap; ++t) {
                if ((match = look(t))) break;
                turn(v, t & 1);
            }
            if (match || t >= turns) break;
            if ((match = look(t))) break;
            resnap(turn0 + t);
            turn(v, t & 1);
            ++t;
        }
        if (match) {
            matched(turn0 + t);
        } else {
            const long long T = turn0 + turns;
            vote(turns & 1);
            // (the workgroup barrier)
            if (agreed(turns & 1)) matched(T);
            else resnap(T);
        }
        if (st.period != 0)
            plain(v, (t + 1) & 1, settle_skip_turns(turn0 + turns - st.settled_turn, st.period));
        else if (snapped)
            store(snap, snaps);
        if (st.period != 0 || snapped) state = st;
        store(v, words);
    }
};

template <int NW, int R>
void settle_host_run(const uint64_t *in, int width, int height, long long turns, int depth,
                     uint64_t *out, int64_t *settled_turn, int64_t *period)
{
    HostSettle<NW, R> h(in, width, height);
    long long turn = 0;
    for (long long left = turns; left > 0;) {
        const int k = settle_next_depth(left, depth);
        h.launch(turn, k);
        turn += k;
        left -= k;
    }
    for (size_t i = 0; i < h.words.size(); ++i) out[i] = h.words[i];
    if (settled_turn) *settled_turn = h.state.settled_turn;
    if (period) *period = h.state.period;
}

using SettleHostRun = void (*)(const uint64_t *, int, int, long long, int, uint64_t *, int64_t *,
                               int64_t *);
SettleHostRun settle_host_run_fn(int nw, int R)
{
    switch (nw * 100 + R) {
    case 101: return settle_host_run<1, 1>;
    case 102: return settle_host_run<1, 2>;
    case 104: return settle_host_run<1, 4>;
    case 108: return settle_host_run<1, 8>;
    case 116: return settle_host_run<1, 16>;
    case 201: return settle_host_run<2, 1>;
    case 202: return settle_host_run<2, 2>;
    case 204: return settle_host_run<2, 4>;
    case 208: return settle_host_run<2, 8>;
    case 301: return settle_host_run<3, 1>;
    case 302: return settle_host_run<3, 2>;
    case 304: return settle_host_run<3, 4>;
    case 305: return settle_host_run<3, 5>;
    case 401: return settle_host_run<4, 1>;
    case 402: return settle_host_run<4, 2>;
    case 404: return settle_host_run<4, 4>;
    default: return nullptr;
    }
}

}  // namespace

hipError_t launch_settle_batch(uint64_t *words, uint64_t *snaps, SettleState *states, int width,
                               int height, int boards, long long turn0, int turns, hipStream_t s)
{
    ResidentPlan p;
    if (!words || !snaps || !states || boards < 1 || turn0 < 0 || turns < 1 ||
        turns > kSettleMaxDepth || (long long)boards * height > INT32_MAX ||
        !resident_plan(width, height, &p))
        return hipErrorInvalidValue;
    void *fn = settle_kernel((width + 63) / 64, p.rows);
    if (!fn) return hipErrorInvalidValue;
    int k = turns;
    void *params[] = {&words, &snaps, &states, &width, &height, &turn0, &k};
    return hipLaunchKernel(fn, dim3((unsigned)boards), dim3(64u * (unsigned)p.waves), params, 0, s);
}

hipError_t launch_settle_init(SettleState *states, int first, int n, long long turn, hipStream_t s)
{
    if (!states || first < 0 || n < 1 || turn < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_settle_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, states,
                       first, n, turn);
    return hipGetLastError();
}

}  // namespace golk

// ================================================================ C ABI (no device)
extern "C" {

int gol_settle_host_run(const uint64_t *in, int32_t width, int32_t height, int64_t turns,
                        int32_t depth, uint64_t *out, int64_t *settled_turn, int64_t *period)
{
    golk::ResidentPlan p;
    if (!in || !out || turns < 0 || depth < 1 || depth > golk::kSettleMaxDepth ||
        !golk::resident_plan(width, height, &p))
        return GOL_EINVAL;
    const golk::SettleHostRun run = golk::settle_host_run_fn((width + 63) / 64, p.rows);
    if (!run) return GOL_EINVAL;
    run(in, width, height, turns, depth, out, settled_turn, period);
    return GOL_OK;
}

}  // extern "C"
