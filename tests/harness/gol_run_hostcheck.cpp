// gol_run_hostcheck.cpp -- a stand-alone program over the public gol_run_* ABI, linked with the
// unmodified csrc/gol_run.cpp and the CPU model of its engine / HIP boundary
// (gol_model_engine.cpp), built plain, with ThreadSanitizer and with AddressSanitizer + UBSan
// (csrc/Makefile `hostcheck`).  Test infrastructure only (tests/test_run_host_cpu.py).
//
// usage: gol_run_hostcheck WORKDIR SCENARIO [ARGS...]
//   full NGPUS HALO CAPACITY         Turns = 25 with TurnComplete
//   keys NGPUS                       unbounded run: s, p, (s, q swallowed), p, q
//   flips bin|nb NGPUS KEYS          CellFlipped, 6 turns; KEYS = 1: s / p land mid-run
//   resume basic|flips|killed|size|env
//   teardown blocked|paused|immediate|misc
//   errors CASE                      see kErrorCases
//   storm NGPUS                      a key thread and a polling thread against the consumer
//   canary race|uaf                  (sanitizer builds only) a deliberate bug on the program's own
//                                    heap, to show that the binary reports
//
// The program writes its input images itself: byte (x, y) of a W x H image of seed s comes from
// mix((s << 32) + y * W + x) (image_byte below; tests/test_run_host_cpu.py has the same
// function).  The "nb" image mixes in bytes that are neither 0 nor 255.
//
// stdout, one line per event, in the format of gol_stub_harness.c plus CellFlipped:
//   RUN <label>                                   a gol_run_start follows
//   StateChange <turn> Executing|Paused|Quitting  AliveCellsCount <turn> <cells>
//   ImageOutputComplete <turn> <name>             TurnComplete <turn>
//   CellFlipped <turn> <x> <y>
//   FinalTurnComplete <turn> <cells>              then: FinalAlive <cells> x y x y ...
//   CLOSED <rc> err=<text>    rc = gol_run_start's code when it failed (text =
//                             gol_run_error(NULL)), else the code that ended the drain
//                             (GOL_ECLOSED; text = gol_run_error(run))
//   DESTROYED                 the run was destroyed before its channel closed
//   CHECK <name> ok           an in-process check of the teardown scenario held
// Exit status 0; 2 for a usage error; 3 with "FAIL ..." when an in-process check failed.
//
// Scenarios are event-driven: the next key goes out when an event arrives.  The only sleep is
// the hold while paused.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "gol_amd.h"

#if defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define HOSTCHECK_TSAN 1
#endif
#if __has_feature(address_sanitizer)
#define HOSTCHECK_ASAN 1
#endif
#endif

namespace {

const int kW = 70, kH = 40;
std::string g_work;
std::mutex g_io;        // one output line at a time
std::mutex g_consume;   // storm: pop + print is one step, so lines keep the channel's order

void say(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::lock_guard<std::mutex> lk(g_io);
    vprintf(fmt, ap);
    putchar('\n');
    fflush(stdout);
    va_end(ap);
}

[[noreturn]] void fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    {
        std::lock_guard<std::mutex> lk(g_io);
        printf("FAIL ");
        vprintf(fmt, ap);
        putchar('\n');
        fflush(stdout);
    }
    va_end(ap);
    _exit(3);
}

#define CHECK(name, cond)                         \
    do {                                          \
        if (!(cond)) fail("%s: %s", name, #cond); \
        say("CHECK %s ok", name);                 \
    } while (0)

uint64_t mix(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// (none of the non-binary values is a whitespace byte: the PGM payload is one "field")
const uint8_t kOdd[6] = {1, 7, 100, 128, 200, 254};

uint8_t image_byte(uint64_t seed, uint64_t index, bool nonbinary)
{
    const uint64_t h = mix((seed << 32) + index);
    if (nonbinary && (h >> 8) % 11 == 0) return kOdd[(h >> 16) % 6];
    return (h & 7) < 3 ? 255 : 0;
}

std::vector<uint8_t> make_image(uint64_t seed, int W, int H, bool nonbinary)
{
    std::vector<uint8_t> b((size_t)W * H);
    for (size_t i = 0; i < b.size(); i++) b[i] = image_byte(seed, i, nonbinary);
    return b;
}

void write_file(const std::string &path, const std::string &head, const uint8_t *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) fail("cannot write %s", path.c_str());
    fwrite(head.data(), 1, head.size(), f);
    if (n) fwrite(p, 1, n, f);
    fclose(f);
}

// WORKDIR/<dir>/<W>x<H>.pgm of the given seed; returns the directory
std::string write_image(const char *dir, uint64_t seed, int W, int H, bool nonbinary)
{
    const std::string d = g_work + "/" + dir;
    ::mkdir(d.c_str(), 0777);
    const std::vector<uint8_t> b = make_image(seed, W, H, nonbinary);
    write_file(d + "/" + std::to_string(W) + "x" + std::to_string(H) + ".pgm",
               "P5\n" + std::to_string(W) + " " + std::to_string(H) + "\n255\n", b.data(),
               b.size());
    return d;
}

struct Spec {
    std::string label = "run";
    int W = kW, H = kH;
    long long turns = 25;
    int ngpus = 1, halo = 0, ticker_ms = 0, capacity = 64;
    bool turn_complete = true, cell_flipped = false;
    int resume = 0;
    std::string image_dir, out_dir;
    std::vector<int32_t> devices;
};

void print_event(gol_run *r, const gol_event &e)
{
    static const char *const state[] = {"Paused", "Executing", "Quitting"};
    switch (e.type) {
    case GOL_EV_STATE_CHANGE:
        say("StateChange %lld %s", (long long)e.completed_turns,
            e.new_state >= 0 && e.new_state <= 2 ? state[e.new_state] : "?");
        break;
    case GOL_EV_ALIVE_CELLS_COUNT:
        say("AliveCellsCount %lld %lld", (long long)e.completed_turns, (long long)e.cells_count);
        break;
    case GOL_EV_IMAGE_OUTPUT_COMPLETE:
        say("ImageOutputComplete %lld %s", (long long)e.completed_turns, e.filename);
        break;
    case GOL_EV_TURN_COMPLETE:
        say("TurnComplete %lld", (long long)e.completed_turns);
        break;
    case GOL_EV_CELL_FLIPPED:
        say("CellFlipped %lld %lld %lld", (long long)e.completed_turns, (long long)e.x,
            (long long)e.y);
        break;
    case GOL_EV_FINAL_TURN_COMPLETE: {
        say("FinalTurnComplete %lld %lld", (long long)e.completed_turns, (long long)e.cells_count);
        const int64_t n = gol_run_final_alive(r, nullptr, 0);
        if (n < 0) fail("gol_run_final_alive after FinalTurnComplete: %lld", (long long)n);
        std::vector<int64_t> xy((size_t)n * 2 + 1);
        if (gol_run_final_alive(r, xy.data(), n) != n) fail("gol_run_final_alive changed");
        std::string line = "FinalAlive " + std::to_string(n);
        for (int64_t i = 0; i < 2 * n; i++) line += " " + std::to_string(xy[(size_t)i]);
        say("%s", line.c_str());
        break;
    }
    default:
        fail("event of unknown type %d", e.type);
    }
}

int start(const Spec &s, gol_run **r)
{
    gol_params p{};
    p.turns = s.turns;
    p.threads = 4;
    p.image_width = s.W;
    p.image_height = s.H;
    gol_run_options o{};
    o.image_dir = s.image_dir.c_str();
    o.out_dir = s.out_dir.c_str();
    o.ngpus = s.ngpus;
    o.devices = s.devices.empty() ? nullptr : s.devices.data();
    o.halo = s.halo;
    o.ticker_ms = s.ticker_ms;
    o.event_capacity = s.capacity;
    o.emit_turn_complete = s.turn_complete;
    o.emit_cell_flipped = s.cell_flipped;
    o.resume = s.resume;
    say("RUN %s", s.label.c_str());
    const int rc = gol_run_start(&p, &o, r);
    if (rc != GOL_OK) say("CLOSED %d err=%s", rc, gol_run_error(nullptr));
    return rc;
}

// one event: pop and print as one step.  Returns gol_run_next_event's code.
int consume(gol_run *r, gol_event &e, int timeout_ms)
{
    std::lock_guard<std::mutex> lk(g_consume);
    const int rc = gol_run_next_event(r, &e, timeout_ms);
    if (rc == GOL_OK) print_event(r, e);
    return rc;
}

using Handler = std::function<void(gol_run *, const gol_event &)>;

void drain(gol_run *r, const Handler &on_event)
{
    gol_event e;
    int rc;
    while ((rc = consume(r, e, -1)) == GOL_OK)
        if (on_event) on_event(r, e);
    say("CLOSED %d err=%s", rc, gol_run_error(r));
    if (gol_run_next_event(r, &e, 0) != GOL_ECLOSED) fail("an event after the channel closed");
}

// start, drain with the handler, destroy; returns gol_run_start's code
int run_one(const Spec &s, const Handler &on_event = nullptr)
{
    gol_run *r = nullptr;
    const int rc = start(s, &r);
    if (rc != GOL_OK) {
        if (r) fail("gol_run_start failed and returned a run");
        return rc;
    }
    drain(r, on_event);
    gol_run_destroy(r);
    return GOL_OK;
}

Spec base_spec(const std::string &image_dir)
{
    Spec s;
    s.image_dir = image_dir;
    s.out_dir = g_work + "/out";
    return s;
}

void hold_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// ----------------------------------------------------------------- scenarios
int scenario_full(int ngpus, int halo, int capacity)
{
    setenv("GOL_MODEL_TURN_US", "300", 0);
    Spec s = base_spec(write_image("img_bin", 1, kW, kH, false));
    s.ngpus = ngpus;
    s.halo = halo;
    s.capacity = capacity;
    s.ticker_ms = 2;
    return run_one(s);
}

// after the first tick s; p; while paused s and q (swallowed); p; after the next tick q
int scenario_keys(int ngpus)
{
    setenv("GOL_MODEL_TURN_US", "100", 0);
    Spec s = base_spec(write_image("img_bin", 1, kW, kH, false));
    s.ngpus = ngpus;
    s.halo = 3;
    s.turns = 1000000000;
    s.ticker_ms = 25;
    s.turn_complete = false;
    int images = 0, states = 0;
    bool started = false, resumed = false, quit = false;
    return run_one(s, [&](gol_run *r, const gol_event &e) {
        if (e.type == GOL_EV_STATE_CHANGE) {
            states++;
            if (e.new_state == GOL_PAUSED) {
                gol_run_key(r, 's');
                gol_run_key(r, 'q');
                hold_ms(90);
                gol_run_key(r, 'p');
            } else if (states > 1 && e.new_state == GOL_EXECUTING) {
                resumed = true;
            }
        } else if (e.type == GOL_EV_IMAGE_OUTPUT_COMPLETE) {
            if (++images == 1) gol_run_key(r, 'p');
        } else if (e.type == GOL_EV_ALIVE_CELLS_COUNT && !started && e.completed_turns > 0) {
            started = true;
            gol_run_key(r, 's');
        } else if (e.type == GOL_EV_ALIVE_CELLS_COUNT && resumed && !quit) {
            quit = true;
            gol_run_key(r, 'q');
        }
    });
}

int scenario_flips(bool nonbinary, int ngpus, bool keys)
{
    // keys: a long turn, so a key sent on an event lands while the next step sleeps before its
    // turn and stops it with no turn done
    setenv("GOL_MODEL_TURN_US", keys ? "3000" : "0", 0);
    const std::vector<uint8_t> img = make_image(nonbinary ? 2 : 1, kW, kH, nonbinary);
    long long alive0 = 0;
    for (uint8_t b : img) alive0 += b == 255;
    Spec s = base_spec(write_image(nonbinary ? "img_nb" : "img_bin", nonbinary ? 2 : 1, kW, kH,
                                   nonbinary));
    s.ngpus = ngpus;
    s.halo = 2;
    s.turns = 6;
    s.cell_flipped = true;
    s.capacity = 8;
    long long seen0 = 0;
    return run_one(s, [&](gol_run *r, const gol_event &e) {
        if (!keys) return;
        if (e.type == GOL_EV_CELL_FLIPPED && e.completed_turns == 0 && ++seen0 == alive0)
            gol_run_key(r, 's');
        else if (e.type == GOL_EV_TURN_COMPLETE && e.completed_turns == 2)
            gol_run_key(r, 'p');
        else if (e.type == GOL_EV_STATE_CHANGE && e.new_state == GOL_PAUSED) {
            hold_ms(10);
            gol_run_key(r, 'p');
        } else if (e.type == GOL_EV_TURN_COMPLETE && e.completed_turns == 4)
            gol_run_key(r, 's');
    });
}

int scenario_resume(const std::string &v)
{
    setenv("GOL_MODEL_TURN_US", "100", 0);
    const std::string dir = write_image("img_bin", 1, kW, kH, false);
    write_image("img_bin", 3, 48, kH, false);
    Spec a = base_spec(dir);
    a.label = "A";
    a.turns = 1000000000;
    a.ticker_ms = 10;
    a.turn_complete = false;
    a.ngpus = v == "flips" ? 3 : 1;
    a.halo = 3;
    const int last = v == "killed" ? 'k' : 'q';
    bool sent = false;
    long long turn_a = 0;
    run_one(a, [&](gol_run *r, const gol_event &e) {
        if (e.type == GOL_EV_ALIVE_CELLS_COUNT && e.completed_turns > 0 && !sent) {
            sent = true;
            gol_run_key(r, last);
        }
        if (e.type == GOL_EV_FINAL_TURN_COMPLETE) turn_a = e.completed_turns;
    });
    Spec b = base_spec(dir);
    b.label = "B";
    b.turns = turn_a + 7;
    b.resume = 1;
    b.ngpus = v == "basic" ? 3 : 1;
    b.halo = 3;
    if (v == "flips") b.cell_flipped = true;
    if (v == "size") b.W = 48;
    if (v == "env") {
        setenv("CONT", "yes", 1);
        b.resume = -1;
    }
    return run_one(b);
}

int scenario_teardown(const std::string &v)
{
    setenv("GOL_MODEL_TURN_US", "100", 0);
    const std::string dir = write_image("img_bin", 1, kW, kH, false);
    gol_run *r = nullptr;
    gol_event e;
    if (v == "blocked") {
        // capacity 1 and a consumer that stops: the driver blocks in send; destroy must end it
        Spec s = base_spec(dir);
        s.turns = 1000;
        s.capacity = 1;
        if (start(s, &r)) return 1;
        for (int i = 0; i < 3; i++)
            if (consume(r, e, -1) != GOL_OK) fail("blocked: channel closed early");
        gol_run_destroy(r);
        say("DESTROYED");
        return 0;
    }
    if (v == "paused") {
        Spec s = base_spec(dir);
        s.turns = 1000000000;
        s.turn_complete = false;
        s.ticker_ms = 5;
        if (start(s, &r)) return 1;
        gol_run_key(r, 'p');
        do {
            if (consume(r, e, -1) != GOL_OK) fail("paused: channel closed early");
        } while (!(e.type == GOL_EV_STATE_CHANGE && e.new_state == GOL_PAUSED));
        gol_run_destroy(r);
        say("DESTROYED");
        return 0;
    }
    if (v == "immediate") {
        Spec s = base_spec(dir);
        s.turns = 1000000000;
        s.capacity = 1;
        if (start(s, &r)) return 1;
        gol_run_destroy(r);
        say("DESTROYED");
        return 0;
    }
    if (v != "misc") return 2;
    // NULL arguments
    gol_params p{};
    p.turns = 1;
    p.image_width = kW;
    p.image_height = kH;
    CHECK("start_null_params", gol_run_start(nullptr, nullptr, &r) == GOL_EINVAL);
    CHECK("start_null_out", gol_run_start(&p, nullptr, nullptr) == GOL_EINVAL);
    CHECK("next_event_null_run", gol_run_next_event(nullptr, &e, 0) == GOL_EINVAL);
    CHECK("key_null_run", gol_run_key(nullptr, 'q') == GOL_EINVAL);
    CHECK("final_alive_null_run", gol_run_final_alive(nullptr, nullptr, 0) == GOL_EINVAL);
    CHECK("error_null_run", gol_run_error(nullptr) != nullptr);
    gol_run_destroy(nullptr);
    // final_alive before and after FinalTurnComplete; key and next_event after the close
    Spec s = base_spec(dir);
    s.turns = 5;
    s.label = "misc";
    if (start(s, &r)) return 1;
    CHECK("next_event_null_event", gol_run_next_event(r, nullptr, 0) == GOL_EINVAL);
    CHECK("final_alive_before", gol_run_final_alive(r, nullptr, 0) == GOL_ESTATE);
    bool checked = false;
    drain(r, [&](gol_run *run, const gol_event &ev) {
        if (ev.type != GOL_EV_FINAL_TURN_COMPLETE) return;
        const int64_t n = gol_run_final_alive(run, nullptr, 0);
        if (n != ev.cells_count || n < 4) fail("final_alive: n = %lld", (long long)n);
        std::vector<int64_t> all((size_t)n * 2);
        gol_run_final_alive(run, all.data(), n);
        const int64_t cap = n / 2, canary = 0x5a5a5a5a5a5a5a5all;
        // exactly cap pairs + 2 canaries on the heap: ASan sees a write one past them, too
        std::vector<int64_t> part((size_t)cap * 2 + 2, canary);
        if (gol_run_final_alive(run, part.data(), cap) != n) fail("final_alive: cap changed n");
        if (part[(size_t)cap * 2] != canary || part[(size_t)cap * 2 + 1] != canary)
            fail("final_alive wrote past cap");
        if (std::memcmp(part.data(), all.data(), (size_t)cap * 2 * sizeof(int64_t)))
            fail("final_alive: the first cap pairs differ");
        checked = true;
    });
    CHECK("final_alive_cap", checked);
    CHECK("final_alive_after_close", gol_run_final_alive(r, nullptr, 0) > 0);
    CHECK("key_after_close", gol_run_key(r, 's') == GOL_OK && gol_run_key(r, 'q') == GOL_OK);
    CHECK("next_event_after_close", gol_run_next_event(r, &e, -1) == GOL_ECLOSED);
    gol_run_destroy(r);   // after CLOSED
    // a 1 ms timeout on a run that has nothing to say (ticker 2 s, no TurnComplete)
    Spec t = base_spec(dir);
    t.label = "timeout";
    t.turns = 1000000000;
    t.turn_complete = false;
    t.ticker_ms = 2000;
    if (start(t, &r)) return 1;
    if (consume(r, e, -1) != GOL_OK) fail("timeout: no first event");
    CHECK("next_event_timeout", gol_run_next_event(r, &e, 1) == GOL_ETIMEDOUT);
    CHECK("next_event_poll", gol_run_next_event(r, &e, 0) == GOL_ETIMEDOUT);
    gol_run_destroy(r);   // mid-run
    say("DESTROYED");
    return 0;
}

struct ErrorCase {
    const char *name;
    const char *inject;   // GOL_MODEL_FAIL, or NULL
    int ngpus;
    long long turns;
    bool turn_complete, cell_flipped;
    int ticker_ms;
    int key;              // sent on the first event, or 0
};
const ErrorCase kErrorCases[] = {
    {"create", "gol_create_ex:2", 3, 5, true, false, 0, 0},
    {"load", "gol_load:2", 3, 5, true, false, 0, 0},
    {"step_first", "gol_step:1", 1, 5, true, false, 0, 0},
    {"step_inflight", "gol_step:4", 1, 50, true, false, 0, 0},
    {"step_inflight_strips", "gol_step:8", 3, 50, true, false, 0, 0},
    {"halo_copy", "gol_copy_halo_from_lower:2", 3, 50, true, false, 0, 0},
    {"snapshot", "gol_snapshot:1", 1, 1000000000, false, false, 5, 0},
    {"snapshot_strips", "gol_snapshot:2", 3, 1000000000, false, false, 5, 0},
    {"read_board", "gol_read_board:1", 1, 1000000000, false, false, 0, 's'},
    {"read_board_final", "gol_read_board:2", 3, 5, true, false, 0, 0},
    {"flipped", "gol_flipped_cells:3", 1, 6, true, true, 0, 0},
    {"alive", "gol_alive_cells:1", 1, 5, true, false, 0, 0},
    {"read_packed", "gol_read_packed:1", 1, 5, true, false, 0, 0},
    {"sync", "gol_sync:1", 1, 5, true, false, 0, 0},
    {"event_create", "hipEventCreateWithFlags:8", 3, 50, true, false, 0, 0},
    {"event_record", "hipEventRecord:8", 3, 50, true, false, 0, 0},
    {"event_sync", "hipEventSynchronize:2", 3, 50, true, false, 0, 0},
    {"host_malloc", "hipHostMalloc:1+", 3, 10, true, true, 0, 0},
    {"device_count", "hipGetDeviceCount:1", 1, 5, true, false, 0, 0},
};

int scenario_errors(const std::string &v)
{
    setenv("GOL_MODEL_TURN_US", "100", 0);
    const std::string head = "P5\n" + std::to_string(kW) + " " + std::to_string(kH) + "\n255\n";
    const std::vector<uint8_t> img = make_image(1, kW, kH, false);
    const std::string bad = g_work + "/img_bad";
    ::mkdir(bad.c_str(), 0777);
    const std::string name = "/" + std::to_string(kW) + "x" + std::to_string(kH) + ".pgm";
    Spec s = base_spec(bad);
    s.turns = 3;
    s.label = v;
    if (v == "missing") return run_one(s), 0;
    const char *heads[][2] = {{"magic", "P2\n70 40\n255\n"},
                              {"width", "P5\n71 40\n255\n"},
                              {"height", "P5\n70 41\n255\n"},
                              {"maxval", "P5\n70 40\n65535\n"}};
    for (auto &h : heads)
        if (v == h[0]) {
            write_file(bad + name, h[1], img.data(), img.size());
            return run_one(s), 0;
        }
    if (v == "short") {
        write_file(bad + name, head, img.data(), img.size() - 1);
        return run_one(s), 0;
    }
    const std::string dir = write_image("img_bin", 1, kW, kH, false);
    s.image_dir = dir;
    if (v == "outdir") {
        write_file(g_work + "/plainfile", "x", nullptr, 0);
        s.out_dir = g_work + "/plainfile/out";
        return run_one(s), 0;
    }
    if (v == "params") {
        Spec q = s;
        q.label = "width1";
        q.W = 1;
        run_one(q);
        q = s;
        q.label = "height0";
        q.H = 0;
        run_one(q);
        q = s;
        q.label = "turns_negative";
        q.turns = -1;
        run_one(q);
        return 0;
    }
    if (v == "ordinal") {
        s.ngpus = 2;
        s.devices = {0, 2};          // the model has devices 0 and 1
        run_one(s);
        s.label = "ordinal_negative";
        s.devices = {-1, 0};
        run_one(s);
        return 0;
    }
    if (v == "peer") {
        setenv("GOL_MODEL_FAIL", "hipDeviceEnablePeerAccess:2", 1);
        s.ngpus = 2;
        s.devices = {0, 1};
        return run_one(s), 0;
    }
    if (v == "peer_query") {
        setenv("GOL_MODEL_FAIL", "hipDeviceCanAccessPeer:1", 1);
        s.ngpus = 2;
        s.devices = {0, 1};
        return run_one(s), 0;
    }
    for (const ErrorCase &c : kErrorCases)
        if (v == c.name) {
            setenv("GOL_MODEL_FAIL", c.inject, 1);
            s.ngpus = c.ngpus;
            s.halo = 3;
            s.turns = c.turns;
            s.turn_complete = c.turn_complete;
            s.cell_flipped = c.cell_flipped;
            s.ticker_ms = c.ticker_ms;
            bool first = true;
            run_one(s, [&](gol_run *r, const gol_event &) {
                if (first && c.key) gol_run_key(r, c.key);
                first = false;
            });
            return 0;
        }
    return 2;
}

int scenario_storm(int ngpus)
{
    setenv("GOL_MODEL_TURN_US", "50", 0);
    Spec s = base_spec(write_image("img_bin", 1, kW, kH, false));
    s.ngpus = ngpus;
    s.halo = 3;
    s.turns = 1000000000;
    s.ticker_ms = 20;
    s.turn_complete = false;
    s.capacity = 4;
    gol_run *r = nullptr;
    if (start(s, &r)) return 1;
    std::atomic<bool> done{false};
    std::thread keys([&] {
        for (int i = 0; i < 60; i++) {
            gol_run_key(r, 's');
            gol_run_key(r, 'p');
            gol_run_key(r, 'p');
        }
        gol_run_key(r, 'q');
    });
    std::thread poll([&] {
        gol_event e;
        while (!done.load()) {
            if (!gol_run_error(r)) fail("storm: gol_run_error returned NULL");
            (void)consume(r, e, 0);
        }
    });
    gol_event e;
    int rc;
    while ((rc = consume(r, e, 2)) == GOL_OK || rc == GOL_ETIMEDOUT) {
    }
    done.store(true);
    keys.join();
    poll.join();
    say("CLOSED %d err=%s", rc, gol_run_error(r));
    gol_run_destroy(r);
    return 0;
}

#if defined(HOSTCHECK_TSAN) || defined(HOSTCHECK_ASAN)
int scenario_canary(const std::string &v)
{
    if (v == "race") {       // two threads, one heap word, no lock
        long *word = new long(0);
        std::thread a([word] { for (int i = 0; i < 100000; i++) *(volatile long *)word += 1; });
        std::thread b([word] { for (int i = 0; i < 100000; i++) *(volatile long *)word += 1; });
        a.join();
        b.join();
        say("canary race %ld", *word);
        delete word;
        return 0;
    }
    if (v == "uaf") {        // read after delete
        long *block = new long[4]();
        delete[] block;
        say("canary uaf %ld", ((volatile long *)block)[1]);
        return 0;
    }
    return 2;
}
#endif

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s WORKDIR SCENARIO ARGS...\n", argv[0]);
        return 2;
    }
    g_work = argv[1];
    ::mkdir(g_work.c_str(), 0777);
    const std::string sc = argv[2], a1 = argv[3];
    auto num = [&](int i) { return i < argc ? atoi(argv[i]) : 0; };
    int rc = 2;
    if (sc == "full" && argc == 6) rc = scenario_full(num(3), num(4), num(5));
    else if (sc == "keys") rc = scenario_keys(num(3));
    else if (sc == "flips" && argc == 6) rc = scenario_flips(a1 == "nb", num(4), num(5) != 0);
    else if (sc == "resume") rc = scenario_resume(a1);
    else if (sc == "teardown") rc = scenario_teardown(a1);
    else if (sc == "errors") rc = scenario_errors(a1);
    else if (sc == "storm") rc = scenario_storm(num(3));
#if defined(HOSTCHECK_TSAN) || defined(HOSTCHECK_ASAN)
    else if (sc == "canary") rc = scenario_canary(a1);
#endif
    if (rc == 2) fprintf(stderr, "%s: unknown scenario %s %s\n", argv[0], sc.c_str(), a1.c_str());
    return rc < 0 ? 0 : rc;
}
