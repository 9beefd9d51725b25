// gol_resident.hip -- K1r2 k_step_resident (gol_resident.h): the kernel, its instantiation table
// and launch, and the two device-free exports gol_resident_plan / gol_resident_host_run; and
// K1r2b k_step_resident_batch, the same body with blockIdx.x choosing one board of a batch
// (gol_batch.cpp), with k_batch_alive.
#include "gol_resident.h"

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "gol_amd.h"

namespace golk {

namespace {

// One workgroup, `turns` turns (uniform: a kernel argument), the standard word layout in and
// out.  Every launched wave runs every turn and reaches every barrier: lanes past the board hold
// zero rows, publish nothing, read lane 0's rows (their results go nowhere) and store nothing.
// CNT: after turn t = 1 .. turns every lane counts its rows, the wave sums by DPP and leaves the
// sum in its LDS word [t - 1][wave]; after the last turn lane t - 1 adds the waves' sums of turn
// t into counts[(t - 1) * kShards + shard] (k_step_tile_cnt's slot convention: the engine
// passes `turns` consecutive, zeroed slots).
template <int NW, int R, bool CNT>
__global__ __launch_bounds__(kResidentMaxLanes) void k_step_resident(
    const uint64_t *__restrict__ in, uint64_t *__restrict__ out,
    unsigned long long *__restrict__ counts, int width, int height, int pitch, int turns)
{
    __shared__ uint64_t xch[resident_xch_words(NW)];
    __shared__ uint32_t csum[CNT ? kResidentMaxTurns * 4 : 1];
    const int lane = (int)threadIdx.x;
    const int lanes = (height + R - 1) / R;
    const bool active = lane < lanes;
    const int mine = resident_rows_of(lane, R, height);
    const int nb = resident_tail_bits(width, NW);
    const uint64_t tail = resident_tail_mask(nb);
    const int ln = active ? resident_north_lane(lane, lanes) : 0;
    const int ls = active ? resident_south_lane(lane, lanes) : 0;
    const size_t row0 = (size_t)lane * R;

    uint64_t v[R][NW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) v[i][j] = i < mine ? in[(row0 + i) * (size_t)pitch + j] : 0ull;

    auto run = [&](auto rag) {
        constexpr bool RAG = decltype(rag)::value;
        for (int t = 0; t < turns; ++t) {
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
            __syncthreads();
            uint64_t north[NW], south[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                north[j] = xch[resident_xch_index(NW, p, 1, j, ln)];
                south[j] = xch[resident_xch_index(NW, p, 0, j, ls)];
            }
            resident_turn<NW, R, RAG>(v, north, south, mine, nb, tail);
            if constexpr (CNT) {
                // wave sum by DPP: inclusive scan within each row of 16 lanes (row_shr 1, 2, 4,
                // 8), then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 / 3:
                // lane 63 of the wave holds the total (at most 64 x 16 x 64 cells)
                uint32_t acc = resident_alive<NW, R, RAG>(v, mine);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x142, 0xa, 0xf, false);
                acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x143, 0xc, 0xf, false);
                if ((lane & 63) == 63) csum[t * 4 + (lane >> 6)] = acc;
            }
        }
    };
    // (uniform: only the board's last lane can own fewer than R rows)
    if (R > 1 && height % R != 0) run(std::true_type{});
    else run(std::false_type{});

#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j)
            if (i < mine) out[(row0 + i) * (size_t)pitch + j] = v[i][j];

    if constexpr (CNT) {
        __syncthreads();
        const int nwaves = (int)blockDim.x >> 6;
        for (int t = lane; t < turns; t += (int)blockDim.x) {
            uint32_t s = 0;
            for (int w = 0; w < nwaves; ++w) s += csum[t * 4 + w];
            if (s)
                atomicAdd(counts + (size_t)t * kShards + (blockIdx.x & (kShards - 1)),
                          (unsigned long long)s);
        }
    }
}

// wave sum by DPP (k_step_resident's sequence): lane 63 of the wave holds the total
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t acc)
{
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x142, 0xa, 0xf, false);
    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x143, 0xc, 0xf, false);
    return acc;
}

// K1r2b: a batch of boards of one shape.  Workgroup b runs `turns` turns (1 .. 256) of board b,
// whose words start at words + b x height x NW (a 64-bit product) with row pitch NW, on
// k_step_resident's turn and with its control flow: every launched wave runs every turn and
// reaches every barrier, lanes past the board publish nothing and store nothing, the ragged last
// lane has its own instantiation of the loop.  (The two kernels stay apart: with the turn loop
// in a __device__ function that both call, the compiler selects 4 to 60 more VALU instructions
// per instantiation for k_step_resident's loop than it does for the kernel as it stands.)
// IN PLACE: the batch has one board buffer and no double buffer.  A lane loads its own rows
// before the first turn and stores the same rows after the last, and no other workgroup touches
// board b, so reading and writing the same words is correct (no __restrict__ pair here).
// CNT: after the last turn lane t (strided by blockDim.x) sums the waves' LDS words of turn t and
// stores the sum, zero or not, to counts[((turn0 + t + 1) % 256) x boards + b] with a plain
// vector store: a board has one owner and a launch at most 256 turns, so the ring needs no
// atomics, no shards and no zeroing.  turn0: the batch's turn before the launch, modulo 256.
template <int NW, int R, bool CNT>
__global__ __launch_bounds__(kResidentMaxLanes) void k_step_resident_batch(
    uint64_t *words, uint32_t *counts, int width, int height, int boards, int turn0, int turns)
{
    __shared__ uint64_t xch[resident_xch_words(NW)];
    __shared__ uint32_t csum[CNT ? kResidentMaxTurns * 4 : 1];
    uint64_t *board = words + (size_t)blockIdx.x * (size_t)height * (size_t)NW;
    const int lane = (int)threadIdx.x;
    const int lanes = (height + R - 1) / R;
    const bool active = lane < lanes;
    const int mine = resident_rows_of(lane, R, height);
    const int nb = resident_tail_bits(width, NW);
    const uint64_t tail = resident_tail_mask(nb);
    const int ln = active ? resident_north_lane(lane, lanes) : 0;
    const int ls = active ? resident_south_lane(lane, lanes) : 0;
    const size_t row0 = (size_t)lane * R;

    uint64_t v[R][NW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) v[i][j] = i < mine ? board[(row0 + i) * (size_t)NW + j] : 0ull;

    auto run = [&](auto rag) {
        constexpr bool RAG = decltype(rag)::value;
        for (int t = 0; t < turns; ++t) {
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
            __syncthreads();
            uint64_t north[NW], south[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                north[j] = xch[resident_xch_index(NW, p, 1, j, ln)];
                south[j] = xch[resident_xch_index(NW, p, 0, j, ls)];
            }
            resident_turn<NW, R, RAG>(v, north, south, mine, nb, tail);
            if constexpr (CNT) {
                const uint32_t acc = wave_sum_dpp(resident_alive<NW, R, RAG>(v, mine));
                if ((lane & 63) == 63) csum[t * 4 + (lane >> 6)] = acc;
            }
        }
    };
    // (uniform: only the board's last lane can own fewer than R rows)
    if (R > 1 && height % R != 0) run(std::true_type{});
    else run(std::false_type{});

#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j)
            if (i < mine) board[(row0 + i) * (size_t)NW + j] = v[i][j];

    if constexpr (CNT) {
        __syncthreads();
        const int nwaves = (int)blockDim.x >> 6;
        for (int t = lane; t < turns; t += (int)blockDim.x) {
            uint32_t s = 0;
            for (int w = 0; w < nwaves; ++w) s += csum[t * 4 + w];
            counts[(size_t)((turn0 + t + 1) & (kResidentMaxTurns - 1)) * (size_t)boards + blockIdx.x] = s;
        }
    }
}

// Alive cells per board: one wavefront per board (workgroup b: board first + b of the launch's
// range), the lanes stride over the board's height x nw words, the wave sums by DPP.
__global__ __launch_bounds__(64) void k_batch_alive(const uint64_t *__restrict__ words,
                                                    uint32_t *__restrict__ out, int board_words)
{
    const uint64_t *board = words + (size_t)blockIdx.x * (size_t)board_words;
    uint32_t n = 0;
    for (int i = (int)threadIdx.x; i < board_words; i += 64)
        n += (uint32_t)__builtin_popcountll(board[i]);
    n = wave_sum_dpp(n);
    if (threadIdx.x == 63) out[blockIdx.x] = n;
}

template <int NW, int R>
void *resident_fn(bool cnt, bool batch)
{
    if (batch)
        return cnt ? reinterpret_cast<void *>(&k_step_resident_batch<NW, R, true>)
                   : reinterpret_cast<void *>(&k_step_resident_batch<NW, R, false>);
    return cnt ? reinterpret_cast<void *>(&k_step_resident<NW, R, true>)
               : reinterpret_cast<void *>(&k_step_resident<NW, R, false>);
}

// the instantiation for (nw, R): every pair of resident_rows_built, as k_step_resident or
// (batch) as k_step_resident_batch
void *resident_kernel(int nw, int R, bool cnt, bool batch = false)
{
    switch (nw * 100 + R) {
    case 101: return resident_fn<1, 1>(cnt, batch);
    case 102: return resident_fn<1, 2>(cnt, batch);
    case 104: return resident_fn<1, 4>(cnt, batch);
    case 108: return resident_fn<1, 8>(cnt, batch);
    case 116: return resident_fn<1, 16>(cnt, batch);
    case 201: return resident_fn<2, 1>(cnt, batch);
    case 202: return resident_fn<2, 2>(cnt, batch);
    case 204: return resident_fn<2, 4>(cnt, batch);
    case 208: return resident_fn<2, 8>(cnt, batch);
    case 301: return resident_fn<3, 1>(cnt, batch);
    case 302: return resident_fn<3, 2>(cnt, batch);
    case 304: return resident_fn<3, 4>(cnt, batch);
    case 305: return resident_fn<3, 5>(cnt, batch);
    case 401: return resident_fn<4, 1>(cnt, batch);
    case 402: return resident_fn<4, 2>(cnt, batch);
    case 404: return resident_fn<4, 4>(cnt, batch);
    default: return nullptr;
    }
}

// the host build of the kernel for one (NW, R): the same functions, lane by lane, two arrays
// for the exchange area
template <int NW, int R>
void host_run(const uint64_t *in, int width, int height, int turns, uint64_t *out, int64_t *counts)
{
    const int lanes = (height + R - 1) / R;
    const int nb = resident_tail_bits(width, NW);
    const uint64_t tail = resident_tail_mask(nb);
    const bool rag = R > 1 && height % R != 0;
    std::vector<uint64_t> xch((size_t)resident_xch_words(NW), 0);
    struct Regs {
        uint64_t v[R][NW];
    };
    std::vector<Regs> regs((size_t)lanes, Regs{});           // every lane's registers
    for (int lane = 0; lane < lanes; ++lane)
        for (int i = 0; i < resident_rows_of(lane, R, height); ++i)
            for (int j = 0; j < NW; ++j) regs[lane].v[i][j] = in[((size_t)lane * R + i) * NW + j];
    for (int t = 0; t < turns; ++t) {
        const int p = t & 1;
        for (int lane = 0; lane < lanes; ++lane) {
            uint64_t (&v)[R][NW] = regs[lane].v;
            const int mine = resident_rows_of(lane, R, height);
            uint64_t last[NW];
            if (rag) resident_last_row<NW, R, true>(v, mine, last);
            else resident_last_row<NW, R, false>(v, mine, last);
            for (int j = 0; j < NW; ++j) {
                xch[resident_xch_index(NW, p, 0, j, lane)] = v[0][j];
                xch[resident_xch_index(NW, p, 1, j, lane)] = last[j];
            }
        }
        // (the workgroup barrier)
        int64_t alive = 0;
        for (int lane = 0; lane < lanes; ++lane) {
            uint64_t (&v)[R][NW] = regs[lane].v;
            const int mine = resident_rows_of(lane, R, height);
            uint64_t north[NW], south[NW];
            for (int j = 0; j < NW; ++j) {
                north[j] = xch[resident_xch_index(NW, p, 1, j, resident_north_lane(lane, lanes))];
                south[j] = xch[resident_xch_index(NW, p, 0, j, resident_south_lane(lane, lanes))];
            }
            if (rag) {
                resident_turn<NW, R, true>(v, north, south, mine, nb, tail);
                alive += resident_alive<NW, R, true>(v, mine);
            } else {
                resident_turn<NW, R, false>(v, north, south, mine, nb, tail);
                alive += resident_alive<NW, R, false>(v, mine);
            }
        }
        if (counts) counts[t] = alive;
    }
    for (int lane = 0; lane < lanes; ++lane)
        for (int i = 0; i < resident_rows_of(lane, R, height); ++i)
            for (int j = 0; j < NW; ++j) out[((size_t)lane * R + i) * NW + j] = regs[lane].v[i][j];
}

using HostRun = void (*)(const uint64_t *, int, int, int, uint64_t *, int64_t *);
HostRun host_run_fn(int nw, int R)
{
    switch (nw * 100 + R) {
    case 101: return host_run<1, 1>;
    case 102: return host_run<1, 2>;
    case 104: return host_run<1, 4>;
    case 108: return host_run<1, 8>;
    case 116: return host_run<1, 16>;
    case 201: return host_run<2, 1>;
    case 202: return host_run<2, 2>;
    case 204: return host_run<2, 4>;
    case 208: return host_run<2, 8>;
    case 301: return host_run<3, 1>;
    case 302: return host_run<3, 2>;
    case 304: return host_run<3, 4>;
    case 305: return host_run<3, 5>;
    case 401: return host_run<4, 1>;
    case 402: return host_run<4, 2>;
    case 404: return host_run<4, 4>;
    default: return nullptr;
    }
}

// GOL_RESIDENT_ROWS=R in the environment (A/B runs; read at every call): that many rows per
// lane instead of the rule's, where the kernel is built for it and the board fits
int rows_request()
{
    const char *v = getenv("GOL_RESIDENT_ROWS");
    return v ? atoi(v) : 0;
}

}  // namespace

hipError_t launch_resident(const StepArgs &a, int turns, hipStream_t s)
{
    ResidentPlan p;
    // the whole board of a torus buffer whose rows lie word by word: nothing else is resident
    if (!resident_turns_ok(turns) || !a.in || !a.out || a.in == a.out || a.row_lo != 0 ||
        a.row_hi != a.modrows || a.nw != (a.width + 63) / 64 || a.pitch < a.nw ||
        !resident_plan(a.width, a.modrows, &p, rows_request()))
        return hipErrorInvalidValue;
    void *fn = resident_kernel(a.nw, p.rows, a.counts != nullptr);
    if (!fn) return hipErrorInvalidValue;
    const uint64_t *in = a.in;
    uint64_t *out = a.out;
    unsigned long long *counts = a.counts;
    int width = a.width, height = a.modrows, pitch = a.pitch, k = turns;
    void *params[] = {&in, &out, &counts, &width, &height, &pitch, &k};
    return hipLaunchKernel(fn, dim3(1), dim3(64u * (unsigned)p.waves), params, 0, s);
}

hipError_t launch_resident_batch(uint64_t *words, uint32_t *counts, int width, int height,
                                 int boards, long long turn0, int turns, hipStream_t s)
{
    ResidentPlan p;
    // (the partition rule's own R: GOL_RESIDENT_ROWS is an engine experiment)
    if (!words || boards < 1 || turn0 < 0 || turns < 1 || turns > kResidentMaxTurns ||
        (long long)boards * height > INT32_MAX || !resident_plan(width, height, &p))
        return hipErrorInvalidValue;
    void *fn = resident_kernel((width + 63) / 64, p.rows, counts != nullptr, true);
    if (!fn) return hipErrorInvalidValue;
    int t0 = (int)(turn0 % kResidentMaxTurns), k = turns;
    void *params[] = {&words, &counts, &width, &height, &boards, &t0, &k};
    return hipLaunchKernel(fn, dim3((unsigned)boards), dim3(64u * (unsigned)p.waves), params, 0, s);
}

hipError_t launch_batch_alive(const uint64_t *words, int board_words, int boards, uint32_t *out,
                              hipStream_t s)
{
    if (!words || !out || board_words < 1 || boards < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_alive, dim3((unsigned)boards), dim3(64), 0, s, words, out, board_words);
    return hipGetLastError();
}

int resident_batch_blocks_per_cu(int width, int height, bool cnt)
{
    ResidentPlan p;
    if (!resident_plan(width, height, &p)) return 0;
    void *fn = resident_kernel((width + 63) / 64, p.rows, cnt, true);
    int n = 0;
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 64 * p.waves, 0) != hipSuccess)
        return 0;
    return n;
}

}  // namespace golk

// ================================================================ C ABI (no device)
extern "C" {

int gol_resident_plan(int32_t width, int32_t height, int32_t *lanes, int32_t *rows_per_lane,
                      int32_t *waves)
{
    golk::ResidentPlan p;
    if (!lanes || !rows_per_lane || !waves || !golk::resident_plan(width, height, &p))
        return GOL_EINVAL;
    *lanes = p.lanes;
    *rows_per_lane = p.rows;
    *waves = p.waves;
    return GOL_OK;
}

int gol_resident_host_run(const uint64_t *in, int32_t width, int32_t height, int32_t turns,
                          uint64_t *out, int64_t *counts)
{
    golk::ResidentPlan p;
    if (!in || !out || turns < 0 || !golk::resident_plan(width, height, &p)) return GOL_EINVAL;
    const golk::HostRun run = golk::host_run_fn((width + 63) / 64, p.rows);
    if (!run) return GOL_EINVAL;
    run(in, width, height, turns, out, counts);
    return GOL_OK;
}

}  // extern "C"
