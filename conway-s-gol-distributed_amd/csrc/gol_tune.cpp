// gol_tune.cpp — the create-time choice of a launch shape by measurement: the k_step_tile
// model and search (boards of every size), the sweep over kernels, depths and bands with its
// launch planner (engines of >= 2^20 words), and the per-process cache of the results.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <tuple>

#include "gol_ctx.h"

namespace goleng {

namespace {

std::mutex g_tune_mu;
std::map<TuneKey, LaunchShape> g_tune;

}  // namespace

bool tune_cache_lookup(const TuneKey &key, LaunchShape *out)
{
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tune.find(key);
    if (it == g_tune.end()) return false;
    *out = it->second;
    return true;
}

void tune_cache_store(const TuneKey &key, const LaunchShape &s)
{
    std::lock_guard<std::mutex> lk(g_tune_mu);
    g_tune[key] = s;
}

// ---------------------------------------------------------------- k_step_tile planning
namespace {

// every segment code a search below can pick is one the product ships (and tests)
template <size_t N>
constexpr bool all_shipped(const int (&codes)[N])
{
    for (int c : codes)
        if (!golk::tile_code_shipped(c)) return false;
    return true;
}

// A board whose width is no multiple of 64 runs k_step_tile across the row seam: the model's
// ranking and the measured search draw their codes from this list alone there (seam_pickable),
// and every one of them has a seam instantiation
constexpr int kSeamSegs[] = {2, 16, 102, 104, 106, 108, 112, 116, 516, 524};
template <size_t N>
constexpr bool all_seam(const int (&codes)[N])
{
    for (int c : codes)
        if (!golk::tile_code_seam(c)) return false;
    return true;
}
static_assert(all_seam(kSeamSegs) && all_shipped(kSeamSegs),
              "a tile code outside golk::kTileSeamCodes");
bool seam_pickable(int width, int seg)
{
    if (width % 64 == 0) return true;
    for (int c : kSeamSegs)
        if (c == seg) return true;
    return false;
}

}  // namespace

// Modelled time per turn of k_step_tile at one shape, fitted to the
// measured shapes of profiles/r03_tile_*.log: a wave issues (SEG + 2) row sums (8 VALU) and
// SEG rules (14 VALU) per turn, at ~2.36 SIMD cycles per instruction (18 full-rate v_bitop3,
// 4 half-rate v_alignbit / DPP moves per row pair); a SIMD shares its issue between its
// resident waves, one wave alone issues at most every ~5 cycles, and each turn adds a barrier
// and the LDS exchange -- cheaper to hide with >= 2 workgroups per CU (~80 % of the issue
// rate and ~700 cycles a turn) than with one (~70 %, ~900).  Residency from the occupancy
// API (the kernel's VGPRs and dynamic LDS).
double tile_model_us(int ncu, int nw, int rows, int K, int th, int tw, int seg, int width)
{
    if (!golk::tile_shape_ok(nw, K, th, tw, seg, width)) return 0;
    const long long tiles = golk::tile_count(nw, rows, th, tw, seg, K);   // (what is launched)
    const int waves = golk::tile_waves(K, th, tw, seg);
    const int wgpc = golk::tile_blocks_per_cu(K, th, tw, seg, width);  // VGPRs, LDS
    if (wgpc <= 0) return 0;
    const long long slots = (long long)ncu * wgpc;
    const long long rounds = (tiles + slots - 1) / slots;
    const long long per_cu = std::min<long long>((tiles + ncu - 1) / ncu, wgpc);
    const double instr = (seg % 100) * 22.0;                           // per wave and turn
    const double issue = (double)(per_cu * waves) * instr * 2.36 / 4.0;
    const bool two = per_cu >= 2;
    const double turn_cyc = std::max(issue / (two ? 0.8 : 0.7), instr * 5.0) + (two ? 700 : 900);
    const double launch_us = rounds * (K * turn_cyc + 2500.0) / 2400.0 + 3.0;
    return launch_us / K;
}

// The shapes the model ranks best for a board of nw words x rows (the best TH and SEG per
// (K, TW)), fastest first.  TW: every width that splits a row into ntx near-equal tiles; TH:
// the tallest tile the workgroup holds (16 waves) and the heights whose tile count fills 1..4
// resident tiles per CU or a few more tile rows.
// cnt: for a count engine's fused launches -- codes with a counted instantiation only.
std::vector<TileShape> tile_candidates(int ncu, int nw, int rows, int keep, bool cnt, int width,
                                       bool big)
{
    // SEG, and SEG + 100 for the interior-rows-first turn order (gol_tile.hip)
    static constexpr int kSegs[] = {2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 48,
                                    106, 108, 112, 116, 124, 132, 140};
    static_assert(all_shipped(kSegs), "a tile code outside golk::kTileCodes");
    std::vector<TileShape> all;
    std::vector<int> tws;
    for (int ntx = 1; ntx <= nw; ++ntx) {
        const int tw = (nw + ntx - 1) / ntx;
        if (tw <= 62 && (tws.empty() || tws.back() != tw)) tws.push_back(tw);
    }
    for (int K : {8, 12, 16, 20, 24, 32}) {
        for (int tw : tws) {
            TileShape best;
            const int C = tw + 2, G = 64 / C;
            const long long ntx = (nw + tw - 1) / tw;
            for (int seg : kSegs) {
                if (cnt && !golk::tile_code_counted(seg)) continue;
                if (!seam_pickable(width, seg) || (big && !golk::tile_code_big(seg))) continue;
                const int thmax = golk::kTileMaxWavesHost * G * (seg % 100) - 2 * K;
                if (thmax < 1) continue;
                std::vector<long long> ntys;
                const long long nty0 = (rows + thmax - 1) / thmax;
                for (long long n = nty0; n < nty0 + 4; ++n) ntys.push_back(n);
                for (int per_cu = 1; per_cu <= 4; ++per_cu)
                    ntys.push_back(std::max(nty0, ((long long)ncu * per_cu + ntx - 1) / ntx));
                for (long long nty : ntys) {
                    const int th = (int)std::max<long long>(1, (rows + nty - 1) / nty);
                    if (big && !golk::tile_big_ok(width, rows, nw, K, th, seg)) continue;
                    const double m = tile_model_us(ncu, nw, rows, K, th, tw, seg, width);
                    if (m > 0 && (best.K == 0 || m < best.model_us)) best = {K, th, tw, seg, m};
                }
            }
            if (best.K) all.push_back(best);
        }
    }
    std::sort(all.begin(), all.end(),
              [](const TileShape &x, const TileShape &y) { return x.model_us < y.model_us; });
    // the model ranks, the autotune decides: keep the list diverse (at most 2 depths per tile
    // width among the first picks)
    std::vector<TileShape> out;
    std::map<int, int> per_tw;
    for (const TileShape &t : all)
        if (per_tw[t.tw]++ < 2 && (int)out.size() < keep) out.push_back(t);
    for (const TileShape &t : all)
        if ((int)out.size() < keep && per_tw[t.tw] > 2) {
            out.push_back(t);
            per_tw[t.tw] = 0;               // (each width once more at most)
        }
    return out;
}

void apply_tile(gol_ctx *c, const TileShape &t)
{
    LaunchShape s;
    s.multi_variant = golk::kMultiTile;
    s.tpl = t.K;
    s.band_multi = t.th;
    s.tile_w = t.tw;
    s.tile_seg = t.seg;
    s.stream_k = c->shape.stream_k;
    s.stream_tw = c->shape.stream_tw;
    s.stream_th = c->shape.stream_th;
    s.stream_seg = c->shape.stream_seg;
    s.tuned_us_per_turn = c->shape.tuned_us_per_turn;
    set_shape(c, std::move(s));
}

namespace {

// Measured search for the k_step_tile shape (coordinate descent over the launch parameters;
// the model above only seeds the widths): from (the best-filled tile width, 8 waves per
// workgroup, K = 32 or the requested depth, SEG 16), improve one parameter at a time -- SEG
// (both turn orders), tile width, waves per workgroup (the tile height follows: the tallest
// tile that many waves hold), K -- and keep each improvement.  The grid sweeps of
// profiles/r03_tile_grid_*.log put the best shapes at 8-wave workgroups (2 per CU) at every
// board size, with SEG from 4-6 (5120^2) to 16-40 (65536^2).  Returns the best measured
// shape (K == 0: none ran) and its time per turn in *us.
TileShape tile_search(gol_ctx *c, int kfix, float *us, int W)
{
    *us = 0.f;
    const int nw = c->nw, rows = c->buf_rows;
    const int width = c->cfg.width;
    const bool seam = width % 64 != 0;               // (one word per lane, the seam codes)
    if (nw % W || (seam && W != 1)) return TileShape{};
    // a count engine searches the codes with a counted instantiation (one word per lane) and
    // times the counted kernel: the counts of each launch's turns go to the ring's first slots
    // (the ring is cleared when the create ends)
    const bool cnt = (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) && c->count_blocking;
    if (cnt && W != 1) return TileShape{};
    const int nl = nw / W;                           // lane columns (W words each)
    struct WOpt { double useful; int tw; };
    std::vector<WOpt> wopt;
    for (int tw = 1; tw <= 62; ++tw) {
        const int G = 64 / (tw + 2);
        const long long ntx = (nl + tw - 1) / tw;
        wopt.push_back({(double)G * tw / 64.0 * nl / (double)(ntx * tw), tw});
    }
    std::sort(wopt.begin(), wopt.end(), [](const WOpt &x, const WOpt &y) {
        return x.useful > y.useful || (x.useful == y.useful && x.tw > y.tw);
    });
    std::vector<int> tws, tws_wide;                  // the 3 best-filled widths; 8 within 80 %
    for (const WOpt &w : wopt) {
        if ((int)tws.size() < 3 && w.useful >= wopt[0].useful * 0.9) tws.push_back(w.tw);
        if ((int)tws_wide.size() < 8 && w.useful >= wopt[0].useful * 0.8) tws_wide.push_back(w.tw);
    }
    static constexpr int kSegs1[] = {2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 48,
                                     106, 108, 112, 116, 124, 132, 140,
                                     203, 204, 206, 208, 212, 216, 224, 232, 240,
                                     506, 512, 516, 524, 612, 616, 624};
    static constexpr int kSegs2[] = {1002, 1003, 1004, 1006, 1008, 1106, 1108, 1204, 1206, 1208};
    static_assert(all_shipped(kSegs1) && all_shipped(kSegs2), "a tile code outside kTileCodes");
    std::vector<int> segs = W == 1 ? std::vector<int>(std::begin(kSegs1), std::end(kSegs1))
                                   : std::vector<int>(std::begin(kSegs2), std::end(kSegs2));
    if (cnt)
        segs.erase(std::remove_if(segs.begin(), segs.end(),
                                  [](int sg) { return !golk::tile_code_counted(sg); }),
                   segs.end());
    if (seam) segs.assign(std::begin(kSeamSegs), std::end(kSeamSegs));
    struct P { int K, wv, tw, seg, th = 0; };          // th > 0: this height (<= wv's)
    auto shape = [&](const P &p) -> TileShape {
        const int G = 64 / (p.tw + 2);
        int th = p.wv * G * (p.seg % 100) - 2 * p.K;
        if (p.th > 0) th = std::min(th, p.th);
        th = std::min(th, rows);
        // (a big engine: the codes of golk::kTileBigCodes, windows the form takes)
        if (c->tile_big && !golk::tile_big_ok(width, rows, c->pitch, p.K, th, p.seg)) return TileShape{};
        if (th < std::min(8, rows) || (cnt && !golk::tile_code_counted(p.seg)) ||
            !seam_pickable(width, p.seg) || !golk::tile_shape_ok(nw, p.K, th, p.tw, p.seg, width))
            return TileShape{};
        return TileShape{p.K, th, p.tw, p.seg, 0};
    };
    golk::StepArgs a = whole_buffer_args(c);
    a.multi_variant = golk::kMultiTile;
    a.counts = cnt ? c->counts : nullptr;
    if (golk::launch_fill_random(c->board[0], c->cfg.width, nw, c->pitch, rows, 0, rows, 12345,
                                 c->stream) != hipSuccess)
        return TileShape{};
    LaunchTimer timer(c->stream);
    if (!timer.ok()) return TileShape{};
    int reps = 16;
    auto time_one = [&](const TileShape &t, int n) -> float {
        a.band = t.th;
        a.tile_w = t.tw;
        a.tile_seg = t.seg;
        const float ms = timer.ms([&] {
            for (int rep = 0; rep < n; ++rep) {
                a.in = c->board[rep & 1];
                a.out = c->board[(rep + 1) & 1];
                if (golk::launch_step_multi(a, t.K, c->stream) != hipSuccess) return false;
            }
            return true;
        });
        return ms / ((float)n * t.K);
    };
    std::map<std::tuple<int, int, int, int>, float> memo;
    auto measure = [&](const P &p) -> float {
        const TileShape t = shape(p);
        if (!t.K) return 0.f;
        auto key = std::make_tuple(t.K, t.th, t.tw, t.seg);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        float best = 0.f;
        for (int pass = 0; pass < 2; ++pass) {      // best of two (clock noise)
            const float v = time_one(t, reps);
            if (v > 0.f && (best == 0.f || v < best)) best = v;
        }
        memo[key] = best;
        if (getenv("GOL_AUTOTUNE_LOG"))
            fprintf(stderr, "autotune tile %dx%d K=%d th=%d tw=%d seg=%d us_per_turn=%.4f\n",
                    c->cfg.width, rows, t.K, t.th, t.tw, t.seg, best * 1000.f);
        return best;
    };
    P cur{kfix > 0 ? kfix : 32, 8, tws.empty() ? 30 : tws[0], W == 1 ? (cnt ? 516 : 16) : 1008};
    // a big engine starts from the 65536^2 pin: 30 lanes x 452 rows of ORD 5 SEG 16 in 16-wave
    // workgroups at K = 30 (the K = 20 pin, 30 x 472, is timed beside it below)
    const bool big_seed = c->tile_big && W == 1 && shape(P{kfix > 0 ? kfix : 30, 16, 30, 516}).K;
    if (big_seed) cur = P{kfix > 0 ? kfix : 30, 16, 30, 516};
    // clock ramp, and the repetitions that make a measurement ~0.5 ms of launches
    {
        TileShape t0 = shape(cur);
        if (!t0.K) {                          // (tiny boards: shallower SEG)
            for (int sg : {8, 4, 2}) {
                // (across the seam: the short seam codes 108, 104, 106)
                cur.seg = seam ? (sg == 2 ? 106 : 100 + sg) : sg + 1000 * (W - 1);
                if ((t0 = shape(cur)).K) break;
            }
        }
        if (t0.K) {
            const float v = time_one(t0, 8) * 1000.f * t0.K;   // us per launch
            if (v > 0.f) reps = std::max(2, std::min(16, (int)(500.f / v) + 1));
            (void)time_one(t0, reps);
        }
    }
    float best = measure(cur);
    auto improve = [&](P p) {
        const float v = measure(p);
        if (v > 0.f && (best == 0.f || v < best * 0.995f)) {
            best = v;
            cur = p;
        }
    };
    if (big_seed && kfix <= 0) improve(P{20, 16, 30, 516});
    if ((long long)nw * rows < (1ll << 23)) {
        // boards up to 16384^2: SEG x width x waves jointly first (one turn order) -- one
        // parameter at a time settled on 5120^2 at 18-word tiles of SEG 8 (0.76 us per turn)
        // while 14 x 128 tiles of SEG 6 ran 0.64 (profiles/r03b_tile_search_5120.log)
        static constexpr int kJoint1[] = {102, 103, 104, 106, 108, 112, 116, 124};
        static constexpr int kJoint2[] = {1102, 1103, 1104, 1106, 1108};
        static_assert(all_shipped(kJoint1) && all_shipped(kJoint2), "tile code outside kTileCodes");
        const P base = cur;
        const int *js = W == 1 ? kJoint1 : kJoint2;
        const int nj = W == 1 ? (int)std::size(kJoint1) : (int)std::size(kJoint2);
        for (int i = 0; i < nj; ++i)
            for (int tw : tws_wide)
                for (int wv : {8, 12, 16}) improve(P{base.K, wv, tw, js[i]});
    } else if (W == 1) {
        // larger boards: the short-segment family on 14-word tiles (4 groups of 16 lanes, 16
        // waves at <= 64 VGPRs: 8 waves per SIMD) -- 11 % faster than 62-word SEG 32 tiles on
        // the 8-strip shape, 8 % slower at 65536^2 (profiles/r03_tile_small_seg_65536.log)
        const P base = cur;
        static constexpr int kShort[] = {104, 106, 206, 108};
        static_assert(all_shipped(kShort), "a tile code outside kTileCodes");
        for (int sg : kShort)
            for (int tw : {14, tws.empty() ? 14 : tws[0]})
                for (int wv : {8, 16}) improve(P{base.K, wv, tw, sg});
        // ... and the 80-VGPR family: ORD 5 (edge sums read back from LDS) at SEG 16-24 holds
        // 6 waves per SIMD -- two 12-wave workgroups per CU, the occupancy at which the
        // stencil's instruction mix issues fastest (tools/calib/valu_issue occupancy: 1.66
        // cycles per instruction against 2.43 at 4 waves); 30 x 536 tiles of SEG 24 ran 34.6
        // us per turn at 65536^2 against 36.3 for the best 4-wave shape
        // (profiles/r04_sweep_65536_ord5.log)
        static constexpr int kSix[] = {524, 624, 516, 616};
        static_assert(all_shipped(kSix), "a tile code outside kTileCodes");
        for (int sg : kSix)
            for (int tw : {tws.empty() ? 30 : tws[0], 14})
                for (int wv : {12, 8}) improve(P{base.K, wv, tw, sg});
    }
    {
        const P base = cur;
        for (int sg : segs) improve(P{base.K, base.wv, base.tw, sg});
    }
    {
        const P base = cur;
        for (int tw : tws) improve(P{base.K, base.wv, tw, base.seg});
    }
    {
        const P base = cur;
        for (int wv : {4, 6, 8, 12, 16}) improve(P{base.K, wv, base.tw, base.seg});
    }
    if (kfix <= 0) {
        const P base = cur;
        for (int K : {12, 16, 20, 24, 32}) improve(P{K, base.wv, base.tw, base.seg});
    }
    {
        // width x waves jointly (the tile height follows both: 5120^2 ran best at 10 words x
        // 12 waves, a width the fill ranking puts 4th, profiles/r03_tile_grid_5.log)
        const P base = cur;
        for (int tw : tws_wide)
            for (int wv : {8, 12, 16}) improve(P{base.K, wv, tw, base.seg});
    }
    {
        const P base = cur;
        for (int sg : segs) improve(P{base.K, base.wv, base.tw, sg});
    }
    // round balance: the tallest tile is not always the best -- 525 tiles on 512 slots run 2
    // rounds (8448-row strips at height 576); shorter tiles that fill the same rounds evenly
    // take fewer waves each.  Try the heights whose tile count just fits 1..4 residency rounds.
    {
        const P base = cur;
        const TileShape t0 = shape(base);
        if (t0.K) {
            const long long ntx = (nl + base.tw - 1) / base.tw;
            for (int r = 1; r <= 4; ++r) {
                for (long long nty = (rows + t0.th - 1) / t0.th; nty <= 4ll * rows; ++nty) {
                    const int th = (int)((rows + nty - 1) / nty);
                    if (th < 8) break;
                    const int wg = golk::tile_blocks_per_cu(base.K, th, base.tw, base.seg, width);
                    if (wg <= 0) continue;
                    if (ntx * nty <= (long long)r * c->ncu * wg) {
                        if (th != t0.th) improve(P{base.K, base.wv, base.tw, base.seg, th});
                        break;
                    }
                }
            }
        }
    }
    // the search kept whatever beat the incumbent by 0.5 % on a best-of-2 timing; shapes
    // within noise of each other can trade places from box to box, so the 4 fastest seen are
    // timed again (best of 3) and the fastest of that final round is the pick
    TileShape pick = best > 0.f ? shape(cur) : TileShape{};
    if (pick.K) {
        std::vector<std::pair<float, TileShape>> top;
        for (const auto &m : memo)
            if (m.second > 0.f)
                top.push_back({m.second, TileShape{std::get<0>(m.first), std::get<1>(m.first),
                                                   std::get<2>(m.first), std::get<3>(m.first), 0}});
        std::sort(top.begin(), top.end(),
                  [](const auto &x, const auto &y) { return x.first < y.first; });
        if (top.size() > 4) top.resize(4);
        // ... and among the shapes within 1 % of the fastest of that round (timing noise from
        // box to box), a fixed order decides -- the deepest K, then the lowest segment code,
        // the widest tile, the tallest -- so two boxes that time the same shapes within noise
        // pick the same one
        std::vector<std::pair<float, TileShape>> fin;
        float fbest = 0.f;
        for (const auto &c2 : top) {
            float v = 0.f;
            for (int pass = 0; pass < 3; ++pass) {
                const float u = time_one(c2.second, reps);
                if (u > 0.f && (v == 0.f || u < v)) v = u;
            }
            if (v > 0.f) {
                fin.push_back({v, c2.second});
                if (fbest == 0.f || v < fbest) fbest = v;
            }
        }
        auto before = [](const TileShape &x, const TileShape &y) {
            return std::make_tuple(-x.K, x.seg, -x.tw, -x.th) < std::make_tuple(-y.K, y.seg, -y.tw, -y.th);
        };
        bool have = false;
        for (const auto &f : fin)
            if (f.first <= 1.01f * fbest && (!have || before(f.second, pick))) {
                pick = f.second;
                best = f.first;
                have = true;
            }
    }
    *us = best * 1000.f;
    return pick;
}

}  // namespace

// Boards below 2^20 words (5120^2: 409 600) cannot fill the GPU with band pipelines: they run
// k_step_tile at the measured-best shape.
void autotune_small(gol_ctx *c)
{
    float us1 = 0.f, us2 = 0.f;
    const TileShape t1 = tile_search(c, 0, &us1, 1);
    const TileShape t2 = tile_search(c, 0, &us2, 2);   // two words per lane (count engines: none)
    const bool two = t2.K && (!t1.K || us2 < us1);
    if (!t1.K && !t2.K) return;
    apply_tile(c, two ? t2 : t1);
    c->shape.tuned_us_per_turn = two ? us2 : us1;
    // (K1p has no counted form, and none for the widths k_step_tile alone blocks)
    if (!(c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) && !c->tile_only) blocks_tune_persist(c);
}

// ---------------------------------------------------------------- autotune_multi
namespace {

struct Cand {
    int var, K, band;
    int tw = 0, seg = 0;                             // k_step_tile shape
};

// the sweep's timing context: whole-buffer launches on the engine's own (junk) boards
struct Bench {
    gol_ctx *c;
    bool cnt;                                        // a count engine
    golk::StepArgs a;
    LaunchTimer timer;
    Bench(gol_ctx *c_, bool cnt_) : c(c_), cnt(cnt_), a(whole_buffer_args(c_)), timer(c_->stream) {}

    void aim(int var, int band, int tw, int seg)
    {
        a.band = band;
        a.multi_variant = var;
        a.tile_w = tw;
        a.tile_seg = seg;
    }
    // time `reps` launches of one candidate on the engine's stream, ms per turn (0 on error)
    float time_one(const Cand &cd, int reps)
    {
        aim(cd.var, cd.band, cd.tw, cd.seg);
        a.counts = cnt && c->count_blocking && cd.var == golk::kMultiTile &&
                           golk::tile_code_counted(cd.seg)
                       ? c->counts
                       : nullptr;
        const float ms = timer.ms([&] {
            for (int rep = 0; rep < reps; ++rep) {
                a.in = c->board[rep & 1];
                a.out = c->board[(rep + 1) & 1];
                if (pg_prepare(c, a, cd.K) != hipSuccess ||
                    golk::launch_step_multi(a, cd.K, c->stream) != hipSuccess)
                    return false;
            }
            return true;
        });
        return ms / ((float)reps * cd.K);
    }
    // one launch sequence the way gol_step runs it: host wall time in us from a synchronised
    // stream to the last launch's completion (0 on error)
    float time_seq(const std::vector<Launch> &sq)
    {
        if (hipStreamSynchronize(c->stream) != hipSuccess) return 0.f;
        const auto t0 = std::chrono::steady_clock::now();
        bool ok = true;
        int rep = 0;
        for (const Launch &L : sq) {
            aim(L.var == golk::kMultiTileStream ? golk::kMultiTile : L.var, L.band, L.tw, L.seg);
            a.in = c->board[rep & 1];
            a.out = c->board[(rep + 1) & 1];
            ++rep;
            if (L.var == golk::kMultiTileStream)
                ok = ok && blocks_launch(c, a, L) == hipSuccess;
            else
                ok = ok && pg_prepare(c, a, L.k) == hipSuccess &&
                     golk::launch_step_multi(a, L.k, c->stream) == hipSuccess;
        }
        ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
        const std::chrono::duration<float, std::micro> d = std::chrono::steady_clock::now() - t0;
        return ok ? d.count() : 0.f;
    }
};

// The candidates: for k_step_tile its measured-best shapes (tile_search), for the band kernels
// every (K, band) of a coarse list plus the bands whose grid just fits 1..4 residency rounds.
std::vector<Cand> multi_candidates(gol_ctx *c, const std::vector<int> &vars, bool tune_k)
{
    std::vector<Cand> cand;
    for (int var : vars) {
        if (var == golk::kMultiTile) {
            // the measured-best tile shape (tile_search), timed again beside the rest
            for (int W : {1, 2}) {
                float us = 0.f;
                const TileShape ts = tile_search(c, tune_k ? 0 : c->shape.tpl, &us, W);
                if (ts.K) cand.push_back({var, ts.K, ts.th, ts.tw, ts.seg});
            }
            continue;
        }
        // K = 7 measured no faster than 6 / 8 on k_step_skew (DESIGN); k_step_wg goes to 16
        std::vector<int> ks = !golk::is_wg_variant(var) ? std::vector<int>{6, 8, 10}
                                                  : std::vector<int>{8, 12, 16};
        if (!tune_k) ks = {c->shape.tpl};
        static const int kBands[] = {16, 20, 24, 32, 40, 48, 64, 96, 137, 192};
        const int lane_dw = golk::multi_lane_dwords(c->multi_words, var);
        for (int K : ks) {
            if (!golk::multi_ok(c->cfg.width, K, var)) continue;
            // plus the bands whose grid just fits 1..4 rounds of resident band pipelines
            // (k_step_skew: one per wave, k_step_wg: one per workgroup; 65536^2 at 4
            // waves/SIMD: 274 -> 4080 of 4096 waves, 137 -> 8160 of 8192)
            std::vector<int> bands(std::begin(kBands), std::end(kBands));
            const long long cap = (long long)c->ncu *
                                  golk::multi_blocks_per_cu(K, c->multi_words, var) *
                                  golk::multi_pipes_per_block(var);
            for (int r = 1; r <= 4 && cap > 0; ++r) {
                // the smallest band whose launch fits r rounds
                for (int b = 16; b <= 1024 && b <= c->cfg.rows; ++b)
                    if (golk::multi_pipes(c->cfg.width, c->cfg.rows, b, lane_dw, var) <= r * cap) {
                        bands.push_back(b);
                        break;
                    }
            }
            if (golk::is_pg_variant(var)) {   // the nearest bands it runs at (golk::pg_ok)
                for (int &b : bands) b = golk::pg_band(K, b, var == golk::kMultiWgPgS);
                bands.erase(std::remove(bands.begin(), bands.end(), 0), bands.end());
            }
            std::sort(bands.begin(), bands.end());
            bands.erase(std::unique(bands.begin(), bands.end()), bands.end());
            for (int band : bands) {
                if (band > c->cfg.rows && band != bands[0]) break;
                cand.push_back({var, K, band});
            }
        }
    }
    return cand;
}

// The timing table t[i] (ms per turn) of cand[i]; returns the launches per measurement.
// The clock ramps over the first milliseconds of load: warm up, then two interleaved
// passes over the candidates, best of the two per candidate (one pass picked bands
// 73 / 137 / 218 at 65536^2 on three runs); each candidate times >= ~1 ms of launches
// (strips of 8192 rows launch in ~50 us).  Then the bands next to the best of each (kernel, K)
// are added and timed the same way.
int time_candidates(Bench &b, std::vector<Cand> &cand, std::vector<float> &t)
{
    const gol_ctx *c = b.c;
    t.assign(cand.size(), 0.f);
    int reps = 3;
    {
        const float us = b.time_one(cand.back(), 12) * 1000.f * cand.back().K;   // per launch
        if (us > 0.f) reps = std::max(3, std::min(24, (int)(1000.f / us) + 1));
    }
    auto measure = [&](size_t from) {
        for (int pass = 0; pass < 2; ++pass)
            for (size_t i = from; i < cand.size(); ++i) {
                const float v = b.time_one(cand[i], reps);
                if (v > 0.f && (t[i] == 0.f || v < t[i])) t[i] = v;
            }
    };
    measure(0);
    // refine: the bands next to the best of each (kernel, K) (the coarse list steps by up to
    // 50 %, and a one-round grid's fill changes with every band: 16384^2 parallelogram K = 16
    // ran 3.35 / 3.25 / 3.70 us per turn at bands 43 / 55 / 67)
    const size_t n0 = cand.size();
    for (size_t j = 0; j < n0; ++j) {
        // the best band of each (kernel, K)
        const int var = cand[j].var;
        int bi = -1;
        for (size_t i = 0; i < n0; ++i)
            if (cand[i].var == var && cand[i].K == cand[j].K && t[i] > 0.f &&
                (bi < 0 || t[i] < t[bi]))
                bi = (int)i;
        if (bi != (int)j || var == golk::kMultiTile) continue;
        const Cand best = cand[bi];
        const int step = golk::is_pg_variant(var) ? golk::kWgU : std::max(2, best.band / 16);
        for (int d : {-2, -1, 1, 2}) {
            int band = best.band + d * step;
            if (golk::is_pg_variant(var))
                band = golk::pg_band(best.K, band, var == golk::kMultiWgPgS);
            if (band < 16 || band > std::max(c->cfg.rows, 16)) continue;
            bool seen = false;
            for (const Cand &x : cand)
                seen |= x.var == var && x.K == best.K && x.band == band;
            if (!seen) {
                cand.push_back({var, best.K, band, 0, 0});
                t.push_back(0.f);
            }
        }
    }
    measure(n0);
    return reps;
}

// Within 1.5 % of the best, the deepest K wins: the same steady rate with fewer launches
// when a run is short (65536^2, 20 turns: K = 10 -> 2 launches, 104.7k GCUPS; K = 8 ->
// 7 + 7 + 6, 100.8k; steady state 36.0 vs 36.2 us/turn).  *pick_t: its time, 0 when nothing
// ran (then the pick is the engine's current shape).
Cand pick_candidate(const gol_ctx *c, const std::vector<Cand> &cand, const std::vector<float> &t,
                    float *pick_t)
{
    float best = 0.f;
    for (size_t i = 0; i < cand.size(); ++i)
        if (t[i] > 0.f && (best == 0.f || t[i] < best)) best = t[i];
    const LaunchShape &s = c->shape;
    Cand pick{s.multi_variant, s.tpl, s.band_multi, s.tile_w, s.tile_seg};
    *pick_t = 0.f;
    for (size_t i = 0; i < cand.size(); ++i) {
        if (t[i] <= 0.f || t[i] > best * 1.015f) continue;
        if (*pick_t == 0.f || cand[i].K > pick.K || (cand[i].K == pick.K && t[i] < *pick_t)) {
            pick = cand[i];
            *pick_t = t[i];
        }
    }
    return pick;
}

// For each kernel, its fastest (K, band) is a family: one launch of every family is timed at
// every depth 2..16 (band_same_rounds; k_step_tile to its deepest), best of 2.
std::vector<LaunchFamily> time_families(Bench &b, const std::vector<int> &vars,
                                        const std::vector<Cand> &cand, const std::vector<float> &t,
                                        int reps)
{
    const gol_ctx *c = b.c;
    std::vector<LaunchFamily> fams;
    for (int var : vars) {
        int bi = -1;
        for (size_t i = 0; i < cand.size(); ++i)
            if (cand[i].var == var && t[i] > 0.f && (bi < 0 || t[i] < t[bi])) bi = (int)i;
        if (bi < 0 || !golk::multi_is_il(c->multi_words, var)) continue;
        LaunchFamily f{var, cand[bi].K, cand[bi].band, cand[bi].tw, cand[bi].seg, {}, {}};
        for (int k = 2; k <= golk::kMaxTurnsPerLaunch; ++k) {
            f.T[k] = 0.f;
            f.band_k[k] = 0;
            // (k_step_wg runs depths 2, 3 as k_step_skew: that family covers them; the
            // tile kernel's depth is a runtime loop: it is timed up to 32)
            if ((k > 16 && var != golk::kMultiTile) || !golk::multi_ok(c->cfg.width, k, var) ||
                (golk::is_wg_variant(var) && k < 4))
                continue;
            f.band_k[k] = band_same_rounds(c, var, f.K, f.band, k);
            for (int pass = 0; pass < 2; ++pass) {
                const float v = b.time_one(Cand{var, k, f.band_k[k], f.tw, f.seg}, reps) * (float)k;
                if (v > 0.f && (f.T[k] == 0.f || v < f.T[k])) f.T[k] = v;
            }
        }
        fams.push_back(f);
    }
    return fams;
}

// plan[r], r <= max_turns: the first launch of the sequence of launches of these families with
// the least total measured time for r turns (k = 0: none; no launch leaves one turn over);
// cost[r]: that total.
std::vector<Launch> plan_dp(const LaunchFamily *fams, size_t nfams, int max_turns,
                            std::vector<float> *cost_out = nullptr)
{
    const float inf = 1e30f;
    std::vector<float> cost(max_turns + 1, inf);
    std::vector<Launch> plan(max_turns + 1, Launch{});
    cost[0] = 0.f;
    for (int r = 2; r <= max_turns; ++r)
        for (size_t fi = 0; fi < nfams; ++fi) {
            const LaunchFamily &f = fams[fi];
            for (int k = 2; k <= std::min(r, golk::kMaxTurnsPerLaunch); ++k) {
                if (f.T[k] <= 0.f || r - k == 1 || cost[r - k] >= inf) continue;
                const float v = cost[r - k] + f.T[k];
                if (v < cost[r]) {
                    cost[r] = v;
                    plan[r] = Launch{k, f.var, f.band_k[k], f.tw, f.seg};
                }
            }
        }
    if (cost_out) *cost_out = std::move(cost);
    return plan;
}

// the launches a plan runs for r turns (empty when it has none that add up to r)
std::vector<Launch> plan_chain(const std::vector<Launch> &pl, int r)
{
    std::vector<Launch> out;
    for (int q = r; q >= 2 && pl[q].k >= 2; q -= pl[q].k) out.push_back(pl[q]);
    int n = 0;
    for (const Launch &L : out) n += L.k;
    if (n != r) out.clear();
    return out;
}

bool same_launches(const std::vector<Launch> &x, const std::vector<Launch> &y)
{
    if (x.size() != y.size()) return false;
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].k != y[i].k || x[i].var != y[i].var || x[i].band != y[i].band ||
            x[i].tw != y[i].tw || x[i].seg != y[i].seg || x[i].blk != y[i].blk)
            return false;
    return true;
}

// Short steps (r <= kSeqMax turns, e.g. the bench's 20-turn call): the DP adds
// back-to-back launch times, but a gol_step of r turns starts from a synchronised
// stream, and two plans within a few % of each other by the sum traded places as the
// bench's single timed call (65536^2 x 20: 2 x k_step_skew K = 10 vs 1 x k_step_tile
// K = 20, profiles/r03b_plan_choice.log).  So for every r the DP's plan, the best plan
// of each family alone and each family's single launch of depth r are timed as whole
// sequences the way gol_step runs them -- host wall time from a synchronised stream
// to the last launch's completion, best of 5, candidates interleaved -- and the
// fastest is kept in seq[r].
std::vector<std::vector<Launch>> time_sequences(Bench &b, const std::vector<LaunchFamily> &fams,
                                                const std::vector<Launch> &plan)
{
    const gol_ctx *c = b.c;
    const LaunchShape &s = c->shape;
    std::vector<std::vector<Launch>> seqs(kSeqMax + 1);
    std::vector<std::vector<Launch>> fam_plan;
    for (const LaunchFamily &f : fams) fam_plan.push_back(plan_dp(&f, 1, kSeqMax));
    for (int r = 2; r <= kSeqMax; ++r) {
        std::vector<std::vector<Launch>> cands;
        auto add = [&](std::vector<Launch> sq) {
            if (sq.empty()) return;
            for (const auto &x : cands)
                if (same_launches(x, sq)) return;
            cands.push_back(std::move(sq));
        };
        add(plan_chain(plan, r));
        // K1q (when tuned): the r turns as one launch of 2 or 3 near-equal blocks --
        // shallower blocks carry fewer halo rows, and the launch starts only once
        if (s.stream_k > 0)
            for (int nb : {2, 3}) {
                const int blk = (r + nb - 1) / nb;
                if (blk >= 4 && golk::tile_stream_ok(c->nw, c->buf_rows, blk, s.stream_th,
                                                     s.stream_tw, s.stream_seg))
                    add({Launch{r, golk::kMultiTileStream, s.stream_th, s.stream_tw,
                                s.stream_seg, blk}});
            }
        for (size_t fi = 0; fi < fams.size(); ++fi) {
            add(plan_chain(fam_plan[fi], r));
            if (r <= golk::kMaxTurnsPerLaunch && fams[fi].T[r] > 0.f)
                add({Launch{r, fams[fi].var, fams[fi].band_k[r], fams[fi].tw, fams[fi].seg}});
        }
        if (cands.size() <= 1) {
            if (!cands.empty()) seqs[r] = cands[0];
            continue;
        }
        std::vector<float> tt(cands.size(), 0.f);
        for (int pass = 0; pass < 5; ++pass)
            for (size_t i = 0; i < cands.size(); ++i) {
                const float v = b.time_seq(cands[i]);
                if (v > 0.f && (tt[i] == 0.f || v < tt[i])) tt[i] = v;
            }
        size_t bi = 0;
        for (size_t i = 1; i < cands.size(); ++i)
            if (tt[i] > 0.f && (tt[bi] == 0.f || tt[i] < tt[bi])) bi = i;
        if (tt[bi] > 0.f) seqs[r] = cands[bi];
        if (getenv("GOL_AUTOTUNE_LOG") && (r == 8 || r == 16 || r == 20 || r == 32))
            for (size_t i = 0; i < cands.size(); ++i) {
                fprintf(stderr, "autotune seq %d turns%s %.1f us =", r,
                        i == bi ? " (pick)" : "", tt[i]);
                for (const Launch &L : cands[i])
                    fprintf(stderr, " %d(var %d, band %d, tile %d,%d, blk %d)", L.k,
                            L.var, L.band, L.tw, L.seg, L.blk);
                fprintf(stderr, "\n");
            }
    }
    return seqs;
}

// GOL_AUTOTUNE_LOG (tools only): the measured tables on stderr
void log_candidates(const gol_ctx *c, const std::vector<Cand> &cand, const std::vector<float> &t,
                    int reps)
{
    if (!getenv("GOL_AUTOTUNE_LOG")) return;
    for (size_t i = 0; i < cand.size(); ++i)
        fprintf(stderr, "autotune %dx%d var=%d K=%d band=%d tile=%d,%d us_per_turn=%.3f "
                "reps=%d\n", c->cfg.width, c->buf_rows, cand[i].var, cand[i].K, cand[i].band,
                cand[i].tw, cand[i].seg, t[i] * 1000.f, reps);
}

void log_plan(const std::vector<LaunchFamily> &fams, const std::vector<Launch> &plan,
              const std::vector<float> &cost)
{
    if (!getenv("GOL_AUTOTUNE_LOG")) return;
    for (const LaunchFamily &f : fams)
        for (int k = 2; k <= golk::kMaxTurnsPerLaunch; ++k)
            if (f.T[k] > 0.f)
                fprintf(stderr, "autotune launch var=%d K=%d band=%d us=%.1f\n", f.var, k,
                        f.band_k[k], f.T[k] * 1000.f);
    for (int r : {8, 16, 20, 32, 64, 128})
        if (r <= kPlanMax) {
            fprintf(stderr, "autotune plan %d turns: %.1f us =", r, cost[r] * 1000.f);
            for (int q = r; q >= 2 && plan[q].k >= 2; q -= plan[q].k)
                fprintf(stderr, " %d(var %d, band %d)", plan[q].k, plan[q].var, plan[q].band);
            fprintf(stderr, "\n");
        }
}

}  // namespace

// Create-time timing sweep of the temporal-blocking kernel, its depth K and its band on
// the engine's own buffers.  The fastest choice depends on grid/residency quantisation and
// on whether the two boards fit the 256 MiB MALL (tools/sweep.py, tools/strip_emulate.py:
// 65536^2 -> k_step_skew K = 8 band 137-274; 16384^2 and 8448-row strips -> k_step_wg
// K = 12), which no closed form captured, so large engines measure.  Both kernels run on
// the interleaved layout and every candidate computes the same bits.  `tune_variant`:
// choose between k_step_skew and k_step_wg (otherwise keep the engine's kernel).
void autotune_multi(gol_ctx *c, bool tune_k, bool tune_variant)
{
    const long long words = (long long)c->buf_rows * c->pitch;
    if (words < (1ll << 20)) return;                 // < 64 Mi cells: keep the defaults
    std::vector<int> vars{c->shape.multi_variant};
    if (tune_variant)
        vars = {golk::kMultiSkewILW16, golk::kMultiWg, golk::kMultiWgHx, golk::kMultiWgPg,
                golk::kMultiWgHxS, golk::kMultiWgPgS, golk::kMultiTile};
    // a count engine's multi-turn launches are k_step_tile's counted form or none: only K1t
    // candidates are timed (with the counts), and no launch plan mixes other kernels in
    const bool cnt = (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) != 0;
    if (cnt && tune_variant && c->count_blocking) vars = {golk::kMultiTile};
    std::vector<Cand> cand = multi_candidates(c, vars, tune_k);
    if (cand.empty()) return;
    if (golk::launch_fill_random(c->board[0], c->cfg.width, c->nw, c->pitch, c->buf_rows, 0,
                                 c->buf_rows, 12345, c->stream) != hipSuccess)
        return;
    Bench b(c, cnt);
    if (!b.timer.ok()) return;
    std::vector<float> t;
    const int reps = time_candidates(b, cand, t);
    log_candidates(c, cand, t, reps);
    float best = 0.f;                                // ms per turn of the pick
    const Cand pick = pick_candidate(c, cand, t, &best);
    // Launch planner (tune_k and tune_variant only: nothing pinned).  Time one launch of every
    // family at every depth, then plan, for every t <= kPlanMax turns, the sequence of launches
    // with the least total measured time (plan_launch).  All candidates run on the
    // interleaved layout, so launches of different kernels mix freely.
    std::vector<Launch> plan;
    std::vector<std::vector<Launch>> seqs;
    float stream_best = 0.f;
    if (tune_k && tune_variant && best > 0.f && !cnt) {
        const std::vector<LaunchFamily> fams = time_families(b, vars, cand, t, reps);
        std::vector<float> cost;
        plan = plan_dp(fams.data(), fams.size(), kPlanMax, &cost);
        const LaunchFamily *tile = nullptr;
        for (const LaunchFamily &f : fams)
            if (f.var == golk::kMultiTile) tile = &f;
        stream_best = blocks_tune_stream(c, b.a, tile, best);   // K1q (tools build)
        seqs = time_sequences(b, fams, plan);
        log_plan(fams, plan, cost);
    }
    LaunchShape s = c->shape;                        // (K1q's shape, if kept, is in it)
    s.multi_variant = pick.var;
    s.tpl = pick.K;
    s.band_multi = pick.band;
    if (pick.var == golk::kMultiTile) {
        s.tile_w = pick.tw;
        s.tile_seg = pick.seg;
    }
    s.plan = std::move(plan);
    s.seq = std::move(seqs);
    s.tuned_us_per_turn = (stream_best > 0.f ? stream_best : best) * 1000.f;
    set_shape(c, std::move(s));
}

}  // namespace goleng
