// gol_stream_model.cpp -- a host model of the HIP streams and events and of the kernel launch
// interface that csrc/gol_step.cpp and csrc/gol_plan.cpp leave undefined, so the unmodified
// planner / gol_step / gol_step_overlap source links into a host-only program (tests/harness/
// gol_step_hostcheck.cpp; csrc/Makefile `stepcheck`, tests/test_step_host_cpu.py).  No HIP
// runtime, one thread.  Test infrastructure only: it stands for what ORDERS the kernels, not for
// the kernels (DESIGN.md "gol_step under a stream model").
//
// Streams, events, waits.  A stream is a queue of nodes; nothing runs when it is enqueued.
// hipEventRecord(e, s) binds e to the last node of s at that moment (to a marker node when s is
// empty or has waits that no node has taken yet, so the event stands behind them as in HIP).
// hipStreamWaitEvent(s, e) makes the next node of s depend on the node e was bound to when the
// wait was called: a later re-record does not move the wait.  A wait on an event that was never
// recorded is a no-op, reported as UNRECORDED_WAIT (gol_step.cpp promises it never happens).
// hipStreamSynchronize / hipEventSynchronize / hipDeviceSynchronize flush: they run every node
// they cover, and every node enqueued later is ordered after the nodes a flush covered.
//
// Kernels.  The models follow the contracts written in csrc/gol_kernels.h, not the kernels:
//   launch_step_multi(a, k, s)  reads rows [row_lo - k, row_hi + k) of a.in modulo modrows,
//                               writes rows [row_lo, row_hi) of a.out k turns later; with
//                               a.counts it adds the per-turn popcounts of rows [cnt_lo, cnt_hi)
//                               (those among its output rows) into k consecutive count slots
//   launch_step(a, fast, s)     the same for one turn, in the standard layout; a blocked mask
//                               is refused (hipErrorInvalidValue)
//   launch_il_convert           really interleaves / de-interleaves every word (even cells in
//                               the low dword, odd cells in the high one)
// The multi-turn model decodes and encodes the interleaved layout whenever multi_is_il says so,
// so a layout mix-up is a wrong board.  All of them compute on cells with plain loops, through
// row_r / row_w, which record the rows the running node really touched: the access sets of the
// race check are what the model read and wrote, not a second statement of the contract.
// hipMemsetAsync is a node that writes the rows (count slots) it clears.  A counted launch's add
// into a slot is recorded as a read and a write of it (the engine never runs two counted
// launches side by side, so the model needs no notion of an atomic add).
//
// Predicates: permissive stand-ins, not the product's rules.  multi_ok and tile_shape_ok are
// true for 2 .. 64 turns on kMultiTile, tile_grid is the rectangular grid with no repack,
// tile_blocks_per_cu is 1, blocks_plan is false, fail stores the text, the rest are trivial.
//
// At every flush and at the end of a run (gsm::finish):
//   1. Race check.  Happens-before = stream order + event edges + host flushes.  For every pair
//      of executed nodes that touched overlapping rows of one buffer, at least one writing,
//      neither ordered before the other:  RACE <node a> <node b> <buffer> <rows>.  Host reads
//      (gsm::host_read) are nodes too.
//   2. Adversarial execution.  The pending nodes run in a legal topological order chosen by the
//      run's policy: issue order; the ready node of the highest-numbered stream; of the lowest;
//      seeded random picks.  Nodes a flush does not cover may run early or stay pending.
//
// Mutation: GOL_MODEL_DROP_WAIT=<n>, <a>-<b> or a comma list of those ignores these
// hipStreamWaitEvent calls of a run (counted from 1; gsm::reset restarts the count, and every
// run of one process issues the same waits).  Each wait prints
//   WAIT <n> launch=<i> stream=<s> event_stream=<t>[ dropped]
// where launch is the engine's count of stencil launches issued so far (gsm::set_hooks).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "gol_ctx.h"

struct ihipStream_t {
    int id = 0;
    std::string name;
    int last = -1;                 // the last node enqueued
    std::vector<int> waits;        // event nodes the next node depends on
};
struct ihipEvent_t {
    int node = -1;                 // the node it was bound to at the last record
    int stream = -1;
    bool recorded = false;
};

namespace gsm {

struct Buffer {
    std::string name;
    const char *base;
    int rows;
    size_t row_bytes;
};
using Bits = std::vector<uint64_t>;
struct Node {
    int id = 0, stream = -1;       // stream -1: the host
    std::string name;
    std::vector<int> deps;
    std::function<void()> fn;
    bool executed = false;
    long created = 0;              // flushes completed when it was enqueued
    long host_done = -1;           // the flush that covered it
    std::map<int, std::pair<Bits, Bits>> acc;   // buffer -> rows read, rows written
};

enum { kIssue = 0, kHigh = 1, kLow = 2, kRandom = 3 };

struct State {
    std::vector<Node> nodes;
    std::vector<ihipStream_t *> streams;
    std::vector<ihipEvent_t *> events;
    std::vector<Buffer> bufs;
    std::vector<char> checked;     // node was executed at the last race check
    std::set<std::pair<int, int>> raced;
    long nflush = 0;
    int policy = kIssue;
    std::mt19937 rng;
    long waits = 0, kernels = 0, races = 0, unrecorded = 0, live_events = 0;
    int running = -1;
    bool il = true;
    std::function<long long()> launches;
    std::function<void(long long)> on_kernel;
    std::vector<std::pair<long, long>> drop;
};
State g;

void parse_drop()
{
    g.drop.clear();
    const char *e = getenv("GOL_MODEL_DROP_WAIT");
    if (!e) return;
    std::string s(e);
    size_t p = 0;
    while (p < s.size()) {
        size_t q = s.find(',', p);
        if (q == std::string::npos) q = s.size();
        const std::string t = s.substr(p, q - p);
        const size_t d = t.find('-');
        const long a = atol(t.c_str());
        const long b = d == std::string::npos ? a : atol(t.c_str() + d + 1);
        if (a > 0) g.drop.push_back({a, b});
        p = q + 1;
    }
}

void reset(int policy, unsigned seed)
{
    for (auto *s : g.streams) delete s;
    for (auto *e : g.events) delete e;
    const bool il = g.il;
    g = State();
    g.il = il;
    g.policy = policy;
    g.rng.seed(seed);
    parse_drop();
}

void set_il(bool il) { g.il = il; }

void set_hooks(std::function<long long()> launches, std::function<void(long long)> on_kernel)
{
    g.launches = std::move(launches);
    g.on_kernel = std::move(on_kernel);
}

hipStream_t stream_create(const char *name)
{
    auto *s = new ihipStream_t;
    s->id = (int)g.streams.size();
    s->name = name;
    g.streams.push_back(s);
    printf("STREAM %d %s\n", s->id, name);
    return s;
}

void add_buffer(const char *name, const void *base, int rows, size_t row_bytes)
{
    g.bufs.push_back({name, (const char *)base, rows, row_bytes});
}

[[noreturn]] void die(const char *what)
{
    printf("MODEL_ERROR %s\n", what);
    fflush(stdout);
    exit(3);
}

// the running node touches `bytes` bytes at p
void touch(const void *p, size_t bytes, bool write)
{
    const char *a = (const char *)p;
    for (size_t b = 0; b < g.bufs.size(); ++b) {
        const Buffer &B = g.bufs[b];
        if (a < B.base || a >= B.base + (size_t)B.rows * B.row_bytes) continue;
        if (a + bytes > B.base + (size_t)B.rows * B.row_bytes) die("access past the end of a buffer");
        if (g.running < 0) die("access outside a node");
        auto &pr = g.nodes[g.running].acc[(int)b];
        Bits &bits = write ? pr.second : pr.first;
        bits.resize(((size_t)B.rows + 63) / 64);
        const size_t r0 = (size_t)(a - B.base) / B.row_bytes;
        const size_t r1 = (size_t)(a + bytes - 1 - B.base) / B.row_bytes;
        for (size_t r = r0; r <= r1; ++r) bits[r / 64] |= 1ull << (r % 64);
        return;
    }
    die("access to memory no buffer holds");
}

const uint64_t *row_r(const uint64_t *base, long long row, int pitch, int nw)
{
    const uint64_t *p = base + row * pitch;
    touch(p, (size_t)nw * 8, false);
    return p;
}

uint64_t *row_w(uint64_t *base, long long row, int pitch, int nw)
{
    uint64_t *p = base + row * pitch;
    touch(p, (size_t)nw * 8, true);
    return p;
}

int enqueue(hipStream_t s, const std::string &what, std::function<void()> fn)
{
    Node n;
    n.id = (int)g.nodes.size();
    n.stream = s ? s->id : -1;
    n.fn = std::move(fn);
    n.created = g.nflush;
    if (s) {
        if (s->last >= 0) n.deps.push_back(s->last);
        for (int w : s->waits) n.deps.push_back(w);
        s->waits.clear();
        s->last = n.id;
    }
    n.name = "n" + std::to_string(n.id) + ":" + what + "@" + (s ? s->name : std::string("host"));
    g.nodes.push_back(std::move(n));
    return g.nodes.back().id;
}

void execute(int id)
{
    Node &n = g.nodes[id];
    g.running = id;
    if (n.fn) n.fn();
    g.running = -1;
    g.nodes[id].executed = true;
    g.nodes[id].fn = nullptr;
}

std::string row_ranges(const Bits &a, const Bits &b)
{
    std::string out;
    const size_t nb = std::min(a.size(), b.size()) * 64;
    long lo = -1;
    for (size_t r = 0; r <= nb; ++r) {
        const bool on = r < nb && ((a[r / 64] & b[r / 64]) >> (r % 64) & 1);
        if (on && lo < 0) lo = (long)r;
        if (!on && lo >= 0) {
            out += (out.empty() ? "" : ",") + std::to_string(lo) + "-" + std::to_string(r - 1);
            lo = -1;
        }
    }
    return out;
}

bool meet(const Bits &a, const Bits &b)
{
    for (size_t i = 0; i < std::min(a.size(), b.size()); ++i)
        if (a[i] & b[i]) return true;
    return false;
}

void race_check()
{
    const size_t n = g.nodes.size(), nw = (n + 63) / 64;
    // reach[b]: the nodes ordered before b (edges always point to an older node)
    std::vector<Bits> reach(n, Bits(nw, 0));
    for (size_t b = 0; b < n; ++b) {
        Bits &R = reach[b];
        auto add = [&](size_t a) {
            R[a / 64] |= 1ull << (a % 64);
            for (size_t i = 0; i < nw; ++i) R[i] |= reach[a][i];
        };
        for (int d : g.nodes[b].deps) add((size_t)d);
        for (size_t a = 0; a < b; ++a)
            if (g.nodes[a].host_done >= 0 && g.nodes[a].host_done <= g.nodes[b].created &&
                !(R[a / 64] >> (a % 64) & 1))
                add(a);
    }
    g.checked.resize(n, 0);
    for (size_t b = 0; b < n; ++b) {
        if (!g.nodes[b].executed) continue;
        for (size_t a = 0; a < b; ++a) {
            if (!g.nodes[a].executed || (g.checked[a] && g.checked[b])) continue;
            if (reach[b][a / 64] >> (a % 64) & 1) continue;
            for (auto &kv : g.nodes[b].acc) {
                auto it = g.nodes[a].acc.find(kv.first);
                if (it == g.nodes[a].acc.end()) continue;
                const Bits &ar = it->second.first, &aw = it->second.second;
                const Bits &br = kv.second.first, &bw = kv.second.second;
                const Bits *x = nullptr, *y = nullptr;
                if (meet(aw, bw)) x = &aw, y = &bw;
                else if (meet(aw, br)) x = &aw, y = &br;
                else if (meet(ar, bw)) x = &ar, y = &bw;
                if (!x || !g.raced.insert({(int)a, (int)b}).second) continue;
                ++g.races;
                printf("RACE %s %s %s %s\n", g.nodes[a].name.c_str(), g.nodes[b].name.c_str(),
                       g.bufs[kv.first].name.c_str(), row_ranges(*x, *y).c_str());
            }
        }
    }
    for (size_t i = 0; i < n; ++i) g.checked[i] = g.nodes[i].executed;
}

// run the nodes `targets` and everything they depend on (empty: every node), then check
void flush(const std::vector<int> &targets, bool all)
{
    const size_t n = g.nodes.size();
    std::vector<char> need(n, 0);
    std::vector<int> stack(targets);
    if (all)
        for (size_t i = 0; i < n; ++i) need[i] = 1;
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        if (i < 0 || need[i]) continue;
        need[i] = 1;
        for (int d : g.nodes[i].deps) stack.push_back(d);
    }
    for (;;) {
        bool left = false;
        for (size_t i = 0; i < n; ++i) left = left || (need[i] && !g.nodes[i].executed);
        if (!left) break;
        std::vector<int> ready;
        for (size_t i = 0; i < n; ++i) {
            if (g.nodes[i].executed) continue;
            bool ok = true;
            for (int d : g.nodes[i].deps) ok = ok && g.nodes[d].executed;
            if (ok) ready.push_back((int)i);
        }
        if (ready.empty()) die("no node is ready: a cycle");
        int pick = ready[0];
        if (g.policy == kRandom) {
            pick = ready[g.rng() % ready.size()];
        } else if (g.policy != kIssue) {
            for (int r : ready) {
                const int a = g.nodes[r].stream, b = g.nodes[pick].stream;
                if (g.policy == kHigh ? a > b : a < b) pick = r;
            }
        }
        execute(pick);
    }
    ++g.nflush;
    for (size_t i = 0; i < n; ++i)
        if (need[i] && g.nodes[i].host_done < 0) g.nodes[i].host_done = g.nflush;
    race_check();
}

// host work that reads rows [row_lo, row_hi) of a buffer now (a read-out, a served job's copy):
// a node ordered after what the flushes so far covered and before everything enqueued later
void host_read(const uint64_t *base, int row_lo, int row_hi, int pitch, int nw, const char *what)
{
    const int id = enqueue(nullptr, what, nullptr);
    g.running = id;
    for (int r = row_lo; r < row_hi; ++r) (void)row_r(base, r, pitch, nw);
    g.running = -1;
    g.nodes[id].executed = true;
    ++g.nflush;
    g.nodes[id].host_done = g.nflush;
    race_check();
}

// the end of a run: everything still pending runs, the last check; live events are reported
void finish()
{
    flush({}, true);
    printf("END nodes=%zu waits=%ld races=%ld unrecorded=%ld live_events=%ld\n", g.nodes.size(),
           g.waits, g.races, g.unrecorded, g.live_events);
    for (auto *s : g.streams) delete s;
    for (auto *e : g.events) delete e;
    g.streams.clear();
    g.events.clear();
}

uint64_t to_il(uint64_t w)
{
    uint64_t o = 0;
    for (int c = 0; c < 64; ++c) o |= (w >> c & 1) << ((c >> 1) + 32 * (c & 1));
    return o;
}

uint64_t from_il(uint64_t w)
{
    uint64_t o = 0;
    for (int c = 0; c < 64; ++c) o |= (w >> ((c >> 1) + 32 * (c & 1)) & 1) << c;
    return o;
}

namespace {

// k turns of rows [row_lo, row_hi) as the contract states them; il: both boards interleaved
void stencil(const golk::StepArgs &a, int k, bool il)
{
    const int W = a.width, nw = a.nw, R = a.row_hi - a.row_lo, H = R + 2 * k;
    if (R <= 0) return;
    std::vector<uint8_t> cur((size_t)H * W), nxt((size_t)H * W), sum3((size_t)H * W);
    for (int i = 0; i < H; ++i) {
        const long long row = (((long long)a.row_lo - k + i) % a.modrows + a.modrows) % a.modrows;
        const uint64_t *p = row_r(a.in, row, a.pitch, nw);
        for (int j = 0; j < nw; ++j) {
            const uint64_t w = il ? from_il(p[j]) : p[j];
            for (int x = 64 * j; x < std::min(W, 64 * j + 64); ++x)
                cur[(size_t)i * W + x] = (uint8_t)(w >> (x % 64) & 1);
        }
    }
    for (int t = 1; t <= k; ++t) {
        // (a row's sums of three neighbouring cells first, then three rows of them)
        for (int i = t - 1; i < H - t + 1; ++i)
            for (int x = 0; x < W; ++x)
                sum3[(size_t)i * W + x] = (uint8_t)(cur[(size_t)i * W + (x + W - 1) % W] +
                                                    cur[(size_t)i * W + x] +
                                                    cur[(size_t)i * W + (x + 1) % W]);
        for (int i = t; i < H - t; ++i)
            for (int x = 0; x < W; ++x) {
                const int self = cur[(size_t)i * W + x];
                const int nb = sum3[(size_t)(i - 1) * W + x] + sum3[(size_t)i * W + x] +
                               sum3[(size_t)(i + 1) * W + x] - self;
                nxt[(size_t)i * W + x] = nb == 3 || (nb == 2 && self);
            }
        cur.swap(nxt);
        if (a.counts) {
            unsigned long long alive = 0;
            for (int r = std::max(a.cnt_lo, a.row_lo); r < std::min(a.cnt_hi, a.row_hi); ++r)
                for (int x = 0; x < W; ++x) alive += cur[(size_t)(r - a.row_lo + k) * W + x];
            unsigned long long *slot = a.counts + (size_t)(t - 1) * golk::kShards;
            touch(slot, golk::kShards * 8, false);
            touch(slot, golk::kShards * 8, true);
            slot[(a.row_lo / 7) % golk::kShards] += alive;
        }
    }
    for (int i = k; i < H - k; ++i) {
        uint64_t *p = row_w(a.out, a.row_lo + (i - k), a.pitch, nw);
        for (int j = 0; j < nw; ++j) {
            uint64_t w = 0;
            for (int x = 64 * j; x < std::min(W, 64 * j + 64); ++x)
                w |= (uint64_t)cur[(size_t)i * W + x] << (x % 64);
            p[j] = il ? to_il(w) : w;
        }
    }
}

hipError_t launch(const golk::StepArgs &a, int k, bool il, hipStream_t s, const char *kind)
{
    if (!s || k < 1 || a.row_lo > a.row_hi) return hipErrorInvalidValue;
    const long long no = g.kernels++;
    const long long L = g.launches ? g.launches() : -1;
    const std::string what = std::string(kind) + std::to_string(k) + "[" +
                             std::to_string(a.row_lo) + "," + std::to_string(a.row_hi) + ")";
    const int id = enqueue(s, what, [a, k, il] { stencil(a, k, il); });
    printf("LAUNCH %lld launch=%lld k=%d rows=%d-%d stream=%d counts=%d node=%d\n", no, L, k,
           a.row_lo, a.row_hi, s->id, a.counts ? 1 : 0, id);
    if (g.on_kernel) g.on_kernel(no);
    return hipSuccess;
}

}  // namespace
}  // namespace gsm

// ================================================================ the HIP calls of gol_step.cpp
extern "C" {

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    *e = new ihipEvent_t;
    gsm::g.events.push_back(*e);
    ++gsm::g.live_events;
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!e) return hipErrorInvalidHandle;
    --gsm::g.live_events;            // (the object lives until gsm::reset: waits hold node ids)
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    if (!e || !s) return hipErrorInvalidHandle;
    if (s->last < 0 || !s->waits.empty()) gsm::enqueue(s, "marker", nullptr);
    e->node = s->last;
    e->stream = s->id;
    e->recorded = true;
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    if (!s || !e) return hipErrorInvalidHandle;
    const long n = ++gsm::g.waits;
    bool dropped = false;
    for (auto &d : gsm::g.drop) dropped = dropped || (n >= d.first && n <= d.second);
    printf("WAIT %ld launch=%lld stream=%d event_stream=%d%s\n", n,
           gsm::g.launches ? gsm::g.launches() : -1ll, s->id, e->stream,
           dropped ? " dropped" : "");
    if (!e->recorded) {
        ++gsm::g.unrecorded;
        printf("UNRECORDED_WAIT %ld stream=%d\n", n, s->id);
        return hipSuccess;
    }
    if (!dropped) s->waits.push_back(e->node);
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s)
{
    if (!s) return hipErrorInvalidHandle;
    if (!s->waits.empty()) gsm::enqueue(s, "marker", nullptr);
    gsm::flush({s->last}, false);
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t e)
{
    if (!e) return hipErrorInvalidHandle;
    gsm::flush({e->recorded ? e->node : -1}, false);
    return hipSuccess;
}

hipError_t hipDeviceSynchronize(void)
{
    gsm::flush({}, true);
    return hipSuccess;
}

hipError_t hipMemsetAsync(void *p, int value, size_t bytes, hipStream_t s)
{
    if (!p || !s) return hipErrorInvalidValue;
    gsm::enqueue(s, "memset", [p, value, bytes] {
        gsm::touch(p, bytes, true);
        memset(p, value, bytes);
    });
    return hipSuccess;
}

hipError_t hipMemset(void *p, int value, size_t bytes)
{
    memset(p, value, bytes);
    return hipSuccess;
}

hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned)
{
    *p = malloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}

hipError_t hipFree(void *p)
{
    free(p);
    return hipSuccess;
}

hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

hipError_t hipSetDevice(int) { return hipSuccess; }

const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "model HIP error"; }

}  // extern "C"

// ================================================================ golk:: (gol_kernels.h)
namespace golk {

const int kVariantDefault = kVariantRing3;

hipError_t launch_step_multi(const StepArgs &a, int turns, hipStream_t s)
{
    if (turns < 2 || turns > kMaxTileTurns || a.blocked) return hipErrorInvalidValue;
    return gsm::launch(a, turns, multi_is_il(a.multi_words, a.multi_variant), s, "multi");
}

hipError_t launch_step(const StepArgs &a, bool, hipStream_t s)
{
    if (a.blocked) return hipErrorInvalidValue;          // (the model has no mask)
    return gsm::launch(a, 1, false, s, "one");
}

hipError_t launch_il_convert(const uint64_t *in, int in_pitch, uint64_t *out, int out_pitch,
                             int nrows, int nw, bool to_il, hipStream_t s)
{
    if (!s || in == out) return hipErrorInvalidValue;
    gsm::enqueue(s, to_il ? "to_il" : "from_il", [=] {
        for (int r = 0; r < nrows; ++r) {
            const uint64_t *p = gsm::row_r(in, r, in_pitch, nw);
            uint64_t *q = gsm::row_w(out, r, out_pitch, nw);
            for (int j = 0; j < nw; ++j) q[j] = to_il ? gsm::to_il(p[j]) : gsm::from_il(p[j]);
        }
    });
    return hipSuccess;
}

bool multi_is_il(int words_per_lane, int) { return gsm::g.il && words_per_lane == 1; }
bool multi_ok(int, int turns, int variant, int) { return variant == kMultiTile && turns >= 2 && turns <= 64; }
bool tile_shape_ok(int, int turns, int tile_h, int tile_w, int, int)
{
    return turns >= 2 && turns <= 64 && tile_h >= 1 && tile_w >= 1;
}
int tile_waves(int, int, int, int) { return 1; }
int tile_blocks_per_cu(int, int, int, int, int) { return 1; }
TileGrid tile_grid(int nw, int rows, int, int tile_h, int tile_w, int)
{
    return TileGrid{(nw + tile_w - 1) / tile_w, (rows + tile_h - 1) / tile_h, 0, 0, 0};
}
int multi_lane_dwords(int words_per_lane, int) { return 2 * words_per_lane; }
int multi_pipes_per_block(int) { return 1; }
int multi_blocks_per_cu(int, int, int) { return 1; }
long long multi_pipes(int, int rows, int band, int, int) { return (rows + band - 1) / band; }

}  // namespace golk

// ================================================================ goleng:: (gol_ctx.h)
namespace goleng {

int fail(gol_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
    return code;
}

bool device_exclusive(int) { return false; }
int check_dev_err(gol_ctx *) { return GOL_OK; }

int sync_checked(gol_ctx *c)
{
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    return GOL_OK;
}

void release_blocked(gol_ctx *c) { c->blocked = nullptr; }
bool blocks_plan(gol_ctx *, int64_t, Launch *) { return false; }
hipError_t blocks_launch(gol_ctx *, const golk::StepArgs &, const Launch &) { return hipErrorNotSupported; }

}  // namespace goleng
