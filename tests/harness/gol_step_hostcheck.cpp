// gol_step_hostcheck.cpp -- gol_step / gol_step_overlap / gol_stream_wait of csrc/gol_step.cpp,
// unmodified, over the stream model of tests/harness/gol_stream_model.cpp (csrc/Makefile
// `stepcheck`; tests/test_step_host_cpu.py runs it and judges its output against the oracle).
//
//   gol_step_hostcheck <workdir> <scenario> <policy | all> [arguments]
//
// <workdir>/in.bin holds the start board as packed rows of width / 64 words (s7: one whole board
// per window, the truth at that window's first turn).  Every policy (issue, high, low, rand1 ..
// rand3) runs the scenario on a fresh engine and writes <workdir>/<policy>.board (more files
// where a scenario reads more than once).  Output, line by line: RUN <policy>, STREAM, LAUNCH,
// WAIT, RACE, UNRECORDED_WAIT (the model's), then per step RC <code>, CHUNKS <n>, TURN <t>,
// LAUNCHES <k> ..., then END (the model's totals).  GOL_STEP_CHUNKS and GOL_MODEL_DROP_WAIT come
// from the environment.
//
// The engine is a gol_ctx filled directly from gol_ctx.h: no gol_create, so no tuner and no
// pinned table.  Boards are 320 cells wide (5 whole words: the model has no seam logic), k_step_tile
// with 5-word tiles at segment code 516, one word per lane.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "gol_ctx.h"

// the model's own interface (gol_stream_model.cpp)
namespace gsm {
void reset(int policy, unsigned seed);
void set_il(bool il);
void set_hooks(std::function<long long()> launches, std::function<void(long long)> on_kernel);
hipStream_t stream_create(const char *name);
void add_buffer(const char *name, const void *base, int rows, size_t row_bytes);
int enqueue(hipStream_t s, const std::string &what, std::function<void()> fn);
const uint64_t *row_r(const uint64_t *base, long long row, int pitch, int nw);
uint64_t *row_w(uint64_t *base, long long row, int pitch, int nw);
void host_read(const uint64_t *base, int row_lo, int row_hi, int pitch, int nw, const char *what);
void finish();
uint64_t to_il(uint64_t w);
uint64_t from_il(uint64_t w);
}  // namespace gsm

using goleng::own_hi;
using goleng::own_lo;

namespace {

constexpr int W = 320, NW = 5, SEG = 516;
std::string g_dir, g_policy;
std::vector<uint64_t> g_in;

[[noreturn]] void usage(const char *why)
{
    fprintf(stderr, "gol_step_hostcheck: %s\n", why);
    exit(2);
}

void load_input()
{
    FILE *f = fopen((g_dir + "/in.bin").c_str(), "rb");
    if (!f) usage("cannot open in.bin");
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) g_in.push_back(w);
    fclose(f);
}

void write_rows(const std::string &name, const std::vector<uint64_t> &rows)
{
    const std::string path = g_dir + "/" + g_policy + "." + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(rows.data(), 8, rows.size(), f) != rows.size()) usage("cannot write a board");
    fclose(f);
}

struct Eng {
    std::unique_ptr<gol_ctx> ctx;
    gol_ctx *c;
    std::vector<uint64_t> b[2];
    std::vector<unsigned long long> counts;
    hipStream_t recv = nullptr;
    std::string tag;

    // a torus engine (halo 0, rows = height) or the strip [row_offset, row_offset + rows)
    Eng(const std::string &tag_, int height, int row_offset, int rows, int halo, unsigned flags,
        int ncu, int tpl, int th)
        : ctx(new gol_ctx), c(ctx.get()), tag(tag_)
    {
        c->cfg.width = W;
        c->cfg.height = height;
        c->cfg.row_offset = row_offset;
        c->cfg.rows = rows;
        c->cfg.halo = halo;
        c->cfg.flags = flags;
        c->cfg.turns_per_launch = tpl;
        c->nw = NW;
        c->pitch = NW + 1;                       // (a padding word per row, never touched)
        c->buf_rows = rows + 2 * halo;
        c->fast = true;
        c->multi_words = 1;
        c->ncu = ncu;
        c->count_blocking = true;
        c->halo_valid = 0;
        for (int i = 0; i < 2; ++i) {
            b[i].assign((size_t)c->buf_rows * c->pitch, 0xA5A5A5A5A5A5A5A5ull);
            c->board[i] = b[i].data();
            gsm::add_buffer((tag + "board" + std::to_string(i)).c_str(), b[i].data(), c->buf_rows,
                            (size_t)c->pitch * 8);
        }
        counts.assign((size_t)(kRingSlots + 1) * kShards, 0);
        c->counts = counts.data();
        gsm::add_buffer((tag + "counts").c_str(), counts.data(), kRingSlots + 1, kShards * 8);
        c->stream = gsm::stream_create((tag + "engine").c_str());
        c->side = gsm::stream_create((tag + "side").c_str());
        if (halo > 0) recv = gsm::stream_create((tag + "recv").c_str());
        (void)hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming);
        goleng::LaunchShape s;
        s.multi_variant = golk::kMultiTile;
        s.tpl = tpl;
        s.band_multi = th;
        s.tile_w = NW;
        s.tile_seg = SEG;
        goleng::set_shape(c, s);
    }
    ~Eng()
    {
        // (gol_engine.cpp is not linked: as gol_destroy, drain the device -- the nodes still
        // pending hold pointers into this engine's boards -- then destroy the engine's events)
        (void)hipDeviceSynchronize();
        for (auto &set : c->chunk_ev)
            for (hipEvent_t &e : set)
                if (e) (void)hipEventDestroy(e);
        (void)hipEventDestroy(c->ev_side);
        (void)hipEventDestroy(c->ev_main);
    }
    int global_row(int buf_row) const
    {
        const int H = c->cfg.height;
        return ((c->cfg.row_offset - c->cfg.halo + buf_row) % H + H) % H;
    }
    // the whole buffer from a packed board of cfg.height rows, standard layout
    void load(const uint64_t *board)
    {
        for (int r = 0; r < c->buf_rows; ++r)
            memcpy(&b[0][(size_t)r * c->pitch], board + (size_t)global_row(r) * NW, NW * 8);
        c->cur = 0;
        c->il = false;
    }
    void report(int rc)
    {
        printf("RC %d\nCHUNKS %lld\nTURN %lld\nLAUNCHES", rc, c->last_chunks, c->turn);
        for (const Launch &L : c->last) printf(" %d", L.k);
        printf("\n");
        if (rc < 0) printf("ERROR %s\n", c->err.c_str());
    }
    void step(int64_t turns) { report(gol_step(c, turns)); }
    // as the engine's read-out does: the standard layout, the engine stream drained, then the
    // host reads the owned rows
    void read(const std::string &name, int half = 0)
    {
        if (goleng::ensure_layout(c, false) != GOL_OK) usage("ensure_layout failed");
        (void)hipStreamSynchronize(c->stream);
        const uint64_t *src = c->board[c->cur ^ half];
        gsm::host_read(src, own_lo(c), own_hi(c), c->pitch, NW, "readout");
        std::vector<uint64_t> out;
        for (int r = own_lo(c); r < own_hi(c); ++r)
            out.insert(out.end(), src + (size_t)r * c->pitch, src + (size_t)r * c->pitch + NW);
        write_rows(name, out);
    }
    unsigned long long count_of(long long turn) const
    {
        unsigned long long v = 0;
        for (int i = 0; i < kShards; ++i) v += counts[(size_t)(turn % kRingSlots) * kShards + i];
        return v;
    }
    // the counts of turns (from, to], read by the host after the engine stream drained
    void read_counts(long long from, long long to, const char *label)
    {
        (void)hipStreamSynchronize(c->stream);
        for (long long t = from + 1; t <= to; ++t) {
            gsm::host_read((const uint64_t *)counts.data(), (int)(t % kRingSlots),
                           (int)(t % kRingSlots) + 1, kShards, kShards, "countread");
            printf("%s %lld %llu\n", label, t, count_of(t));
        }
    }
    // what run_read does while a step is in progress
    void post(Job *j)
    {
        std::lock_guard<std::mutex> jl(c->jm);
        c->jobs.push_back(j);
        c->jobs_pending.store(true);
        c->readers.store(true);
    }
    // "on the first kernel of launch n, run this"
    void at_launch(long long n, std::function<void()> fn)
    {
        auto fired = std::make_shared<bool>(false);
        gol_ctx *cc = c;
        gsm::set_hooks([cc] { return cc->launches; }, [cc, n, fn, fired](long long) {
            if (cc->launches == n && !*fired) {
                *fired = true;
                fn();
            }
        });
    }
    void watch()
    {
        gol_ctx *cc = c;
        gsm::set_hooks([cc] { return cc->launches; }, nullptr);
    }
};

int arg_int(const std::vector<std::string> &a, size_t i)
{
    if (i >= a.size()) usage("too few arguments");
    return atoi(a[i].c_str());
}

// ---------------------------------------------------------------- scenarios
// s1 <rows> <turns> <tpl>, s3 <rows> <turns> <tpl> <ncu>: one step on a torus of 40-row tiles
void s_step(const std::vector<std::string> &a, bool with_ncu)
{
    const int rows = arg_int(a, 0), turns = arg_int(a, 1), tpl = arg_int(a, 2);
    Eng e("", rows, 0, rows, 0, 0, with_ncu ? arg_int(a, 3) : 1, tpl, 40);
    e.watch();
    e.load(g_in.data());
    e.step(turns);
    e.read("board");
}

// s2 <seq | plan>: 640 rows, 17 turns as 6 turns on 40-row tiles, 5 on 48, 6 on 32
void s2(const std::vector<std::string> &a)
{
    if (a.empty()) usage("s2 <seq | plan>");
    Eng e("", 640, 0, 640, 0, 0, 1, 6, 40);
    e.watch();
    goleng::LaunchShape s = e.c->shape;
    const Launch l0{6, golk::kMultiTile, 40, NW, SEG}, l1{5, golk::kMultiTile, 48, NW, SEG},
        l2{6, golk::kMultiTile, 32, NW, SEG};
    if (a[0] == "seq") {
        s.seq.resize(kSeqMax + 1);
        s.seq[17] = {l0, l1, l2};
    } else {
        s.plan.assign(kPlanMax + 1, Launch{});
        s.plan[17] = l0;
        s.plan[11] = l1;
        s.plan[6] = l2;
    }
    goleng::set_shape(e.c, s);
    e.load(g_in.data());
    e.step(17);
    e.read("board");
}

// s4 <tail | two | one | lone>
void s4(const std::vector<std::string> &a)
{
    if (a.empty()) usage("s4 <variant>");
    const std::string v = a[0];
    const int rows = v == "two" ? 270 : 203;
    Eng e("", rows, 0, rows, 0, 0, 1, v == "tail" ? 2 : 6, 40);
    e.watch();
    e.load(g_in.data());
    if (v == "tail") {
        e.step(5);                               // 2, 2, 1
        e.read("board");
    } else if (v == "two") {
        setenv("GOL_STEP_CHUNKS", "3", 1);
        e.step(23);
        e.read("mid.board");
        setenv("GOL_STEP_CHUNKS", "5", 1);
        e.step(12);
        e.read("board");
    } else if (v == "one") {
        e.step(23);
        e.step(1);
        printf("PREV_VALID %d\n", e.c->prev_valid ? 1 : 0);
        e.read("board");
        e.read("prev.board", 1);
    } else if (v == "lone") {
        e.step(6);
        e.read("board");
    } else {
        usage("s4: unknown variant");
    }
}

// s5: a reader's job posted at launch 2 of the 4 launches of a chunked 23-turn step
void s5()
{
    Eng e("", 270, 0, 270, 0, 0, 1, 6, 40);
    gol_ctx *c = e.c;
    Job job;
    job.fn = [c] {
        // the whole current board through the engine stream, then the host waits for it
        auto copy = std::make_shared<std::vector<uint64_t>>();
        const uint64_t *src = c->board[c->cur];
        const int rows = c->buf_rows, pitch = c->pitch;
        gsm::enqueue(c->stream, "jobcopy", [copy, src, rows, pitch] {
            for (int r = 0; r < rows; ++r) {
                const uint64_t *p = gsm::row_r(src, r, pitch, NW);
                copy->insert(copy->end(), p, p + NW);
            }
        });
        if (hipStreamSynchronize(c->stream) != hipSuccess) return GOL_EHIP;
        if (c->il)
            for (uint64_t &w : *copy) w = gsm::from_il(w);
        printf("JOB turn=%lld launches=%lld\n", c->turn, c->launches);
        write_rows("job.board", *copy);
        return GOL_OK;
    };
    e.at_launch(2, [&] { e.post(&job); });
    e.load(g_in.data());
    e.step(23);
    printf("JOBDONE %d rc=%d\n", job.done ? 1 : 0, job.rc);
    e.read("board");
}

// s6: an engine under a control word; STOP stored at launch 2
void s6()
{
    Eng e("", 270, 0, 270, 0, 0, 1, 6, 40);
    (void)gol_set_control(e.c, GOL_CONTROL_RUN);
    e.at_launch(2, [&] { (void)gol_set_control(e.c, GOL_CONTROL_STOP); });
    e.load(g_in.data());
    e.step(23);
    e.read("board");
}

// s7 <form> <strips> <window turns>...: strip engines with 11-row halos, one after the other,
// each window's halos received on a third stream from the truth board of that window
void s7(const std::vector<std::string> &a)
{
    if (a.size() < 3) usage("s7 <form> <strips> <turns>...");
    const std::string form = a[0];
    const int strips = arg_int(a, 1), halo = 11;
    const int rows = form == "short" ? 12 : 40, height = rows * strips;
    const bool cnt = form == "count";
    std::vector<int> windows;
    for (size_t i = 2; i < a.size(); ++i) windows.push_back(arg_int(a, i));
    if (g_in.size() != windows.size() * (size_t)height * NW) usage("s7: in.bin has another size");
    for (int sidx = 0; sidx < strips; ++sidx) {
        Eng e("s" + std::to_string(sidx) + ".", height, sidx * rows, rows, halo,
              cnt ? GOL_FLAG_COUNT_EVERY_TURN : 0u, 1, form == "one" ? 1 : 6, 40);
        gol_ctx *c = e.c;
        e.watch();
        e.load(g_in.data());
        for (size_t wi = 0; wi < windows.size(); ++wi) {
            // as gol_halo_buffers: the board in the layout the first launch after a full
            // exchange runs on, then the receives into its halo rows, behind the engine's work
            if (goleng::ensure_layout(c, goleng::stepping_il(c, goleng::plan_launch(c, halo).k)))
                usage("ensure_layout failed");
            if (gol_stream_wait(c, e.recv) != GOL_OK) usage("gol_stream_wait failed");
            const uint64_t *truth = g_in.data() + wi * (size_t)height * NW;
            uint64_t *dst = c->board[c->cur];
            const bool il = c->il;
            const int pitch = c->pitch;
            for (int part = 0; part < 2; ++part) {
                const int lo = part ? own_hi(c) : 0, hi = part ? c->buf_rows : own_lo(c);
                std::vector<int> grow;
                for (int r = lo; r < hi; ++r) grow.push_back(e.global_row(r));
                gsm::enqueue(e.recv, part ? "recv_bottom" : "recv_top",
                             [truth, dst, il, pitch, lo, hi, grow] {
                                 for (int r = lo; r < hi; ++r) {
                                     uint64_t *p = gsm::row_w(dst, r, pitch, NW);
                                     for (int j = 0; j < NW; ++j) {
                                         const uint64_t w = truth[(size_t)grow[r - lo] * NW + j];
                                         p[j] = il ? gsm::to_il(w) : w;
                                     }
                                 }
                             });
            }
            e.report(gol_step_overlap(c, windows[wi], e.recv));
        }
        if (cnt) e.read_counts(0, c->turn, ("COUNT" + std::to_string(sidx)).c_str());
        e.read("s" + std::to_string(sidx) + ".board");
    }
}

// s8 <turn0> <turns>: a counted torus engine whose turn counter starts at turn0; a reader's job
// at launch 2 looks at every slot of the window gol_turn_counts accepts
void s8(const std::vector<std::string> &a)
{
    const long long turn0 = arg_int(a, 0);
    const int turns = arg_int(a, 1);
    Eng e("", 203, 0, 203, 0, GOL_FLAG_COUNT_EVERY_TURN, 1, 6, 40);
    gol_ctx *c = e.c;
    c->turn = turn0;
    // every slot holds an older turn's count: never zero
    for (int s = 0; s < kRingSlots; ++s) e.counts[(size_t)s * kShards + 1] = 1000000 + s;
    Job job;
    job.fn = [&e, c, turn0] {
        if (hipStreamSynchronize(c->stream) != hipSuccess) return GOL_EHIP;
        long long nonzero = 0;
        const long long lo = std::max(0ll, c->turn - kRing + 1);
        // (one host read per stretch of slots: the window wraps the ring at most once)
        for (long long t = lo; t <= c->turn;) {
            const long long n = std::min<long long>(c->turn - t + 1, kRingSlots - t % kRingSlots);
            gsm::host_read((const uint64_t *)e.counts.data(), (int)(t % kRingSlots),
                           (int)(t % kRingSlots + n), kShards, kShards, "jobcount");
            t += n;
        }
        for (long long t = lo; t <= c->turn; ++t) {
            if (e.count_of(t) == 0) printf("JOBZERO %lld\n", t);
            else ++nonzero;
            if (t > turn0) printf("JOBCOUNT %lld %llu\n", t, e.count_of(t));
        }
        printf("JOB turn=%lld launches=%lld window=%lld-%lld nonzero=%lld\n", c->turn, c->launches,
               lo, c->turn, nonzero);
        return GOL_OK;
    };
    e.at_launch(2, [&] { e.post(&job); });
    e.load(g_in.data());
    e.step(turns);
    printf("JOBDONE %d rc=%d\n", job.done ? 1 : 0, job.rc);
    e.read_counts(turn0, turn0 + turns, "COUNT");
    e.read("board");
}

void run_scenario(const std::string &sc, const std::vector<std::string> &a)
{
    if (sc == "s1") s_step(a, false);
    else if (sc == "s2") s2(a);
    else if (sc == "s3") s_step(a, true);
    else if (sc == "s4") s4(a);
    else if (sc == "s5") s5();
    else if (sc == "s6") s6();
    else if (sc == "s7") s7(a);
    else if (sc == "s8") s8(a);
    else usage("unknown scenario");
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) usage("usage: gol_step_hostcheck <workdir> <scenario> <policy | all> [arguments]");
    g_dir = argv[1];
    const std::string sc = argv[2], pol = argv[3];
    std::vector<std::string> args(argv + 4, argv + argc);
    load_input();
    const char *names[] = {"issue", "high", "low", "rand1", "rand2", "rand3"};
    const char *chunks_env = getenv("GOL_STEP_CHUNKS");
    const std::string chunks0 = chunks_env ? chunks_env : "";
    bool any = false;
    for (int p = 0; p < 6; ++p) {
        if (pol != "all" && pol != names[p]) continue;
        any = true;
        g_policy = names[p];
        printf("RUN %s\n", names[p]);
        if (chunks_env) setenv("GOL_STEP_CHUNKS", chunks0.c_str(), 1);   // (s4 two changes it)
        gsm::reset(p < 3 ? p : 3, (unsigned)p);
        gsm::set_il(true);
        run_scenario(sc, args);                  // (the engine is gone before the last check:
        gsm::finish();                           //  its events count as destroyed)
        fflush(stdout);
    }
    if (!any) usage("unknown policy");
    return 0;
}
