// tsg_plan.cpp -- the per-call planner (tsg_plan.h): every rule that decides
// what a call with M rows runs, with the measurements behind each threshold.
// Top to bottom: the rules (far X^T, direct X, 64 or 128 rows, the shape, the
// touch settings, the tile map, the small-M walks), then what tsg_plan.h
// exports: the shape indices, x_direct, may_fall_back, plan_call and the
// host-pointer pipeline's chunks.
#include "tsg_plan.h"

#include <algorithm>
#include <cstdlib>

#include "tsg_internal.h"

namespace tsg {

namespace {

// Largest M the automatic choice sends to the small-M (ELL) kernel (see
// pick_ell_variant), the variant with 8-row tiles, and the M up to which
// 8-row tiles are used.
constexpr int kEllAutoMaxM = 32;
constexpr int kEllAutoMaxMChunked = 16;
constexpr int64_t kEllPcRowsMaxMN = 32768;
constexpr int kEllStarvedMaxM = 1024;
constexpr int kEllSmallWMaxM = 128;          // small W: the walk up to this M ...
constexpr double kEllSmallWWork = 420e6;     // ... while M x nnz stays below this
// M up to which the automatic choice always takes the 64-row image, and the
// filled fraction of its last round below which the 128-row image's widest
// shape loses to it (pick_rows64)
constexpr int kRows64AutoMaxM = 512;
constexpr double kRows64FullRound = 0.9;
constexpr int64_t kJitFullWgs = 230;
constexpr int64_t kJitOneRoundWgs = 256;  // one jit workgroup per CU (144 KiB of LDS)
constexpr double kFarXtBytes = 768.0 * 1024 * 1024;  // X^T >= 3x the 256 MiB Infinity Cache
constexpr double kFarCodeBytes = 160.0 * 1024 * 1024;  // code image well inside it
constexpr double kFarKeepXtBytes = 1536.0 * 1024 * 1024;  // X^T >= 6x it: the far image beats the staged 64-row one
constexpr double kXDirectMinAddsPerRow = 32.0;  // 64-row image: direct X from width x density >= this
constexpr int64_t kEllStarvedWgs = 64;
constexpr double kXTouchMaxXBytes = 384.0 * 1024 * 1024;        // pick_xtouch
constexpr double kXTouchDenseMaxXBytes = 1024.0 * 1024 * 1024;  // (dense W)
// the 64-row image's step when it cannot read X directly: its X^T staging
// launch (tsg_transpose_rows_kernel) ahead of the image, at the walk's M
// (X <= 20 MB) -- r06_staged_floor_ab.jsonl
constexpr double kStagedXtUs = 5.0;
static_assert(kEllTileM[kEllTile8] == 8, "kEllTile8 is the 8-row tile");

// Shape (stream width x waves per workgroup) for a call with M rows.  Every
// shape walks the same X^T chunks; a wider stream reads fewer LDS bytes per
// add (32 / width: an X pair read feeds width x 2 rows x d adds), and a
// workgroup needs a CU.  Rule (measured, profiles/r02w4_waves_ab.txt,
// r02_ref_cases.jsonl): the widest stream among the shapes that still give
// >= 230 workgroups (~90% of the CUs: (16000, 1024, 1024) runs 64 x 8 on 250,
// 0.116 ms, not 32 x 8 on 500, 0.141 ms), 8 waves before 4 at equal width;
// if none does, the most workgroups.  configs[1]
// (M = 512, N = 4096): 16 columns x 4 waves, 0.105 ms (8 x 8: 0.120);
// M = 256, N = 16384: 32 x 4, 0.153 ms (16 x 8: 0.173); M >= 1024: 64 x 8.
// A pinned width (tcsc_hip_set_jit_width) runs 8 waves; TSG_JIT_WAVES=4 forces
// 4 waves for every narrow width (diagnostic).
// The far-X^T image (no code touches, non-temporal X^T staging) for 64-wide
// calls on the 1 x 32 tile map (long streams: K >= 8192, density > 3/16, more
// than 4 column and 8 M tiles, pick_jit_map) whose X^T is far larger than the
// 256 MiB Infinity Cache while the code fits in it: the X^T stream then no
// longer evicts the code that every M tile of the XCD re-reads
// (profiles/r03e_far_ab.txt, r03e_long_k_ab.txt, r03e_big_ab.txt, kernel ms):
// (64000, 16384, 4096) s = 4 25.3-26.2 -> 21.6-22.2, (32000, 16384, 4096)
// 12.3-12.4 -> 10.8-10.9, (16000, 16384, 4096) 5.9-6.1 -> 5.35-5.43,
// (64000, 8192, 4096) 11.4-11.8 -> 10.8-10.9; it loses where X^T fits the
// cache ((4096, 16384, 4096) 1.17 -> 1.50, (8192, ...) 2.63 -> 2.77), where
// the code does not (s = 2: 38.9 -> 42.0) and on sparse W (s = 8 / 16: 4.9-9%
// slower; those run the 4 x 8 map).  TSG_JIT_FAR=0/1 overrides.
bool far_xt(const PlanInput &in, int M)
{
    static const int env = [] { const char *e = knob_value("TSG_JIT_FAR"); return e ? atoi(e) : -1; }();
    if (in.B || in.far_mode == 1) return false;
    if (in.far_mode == 2) return true;
    if (in.jit_force) return false;
    if (env >= 0) return env > 0;
    const double nnz = (double)in.nnz, density = nnz / std::max(1.0, (double)in.K * in.N);
    const int64_t mtiles = ((int64_t)M + kJitTileM - 1) / kJitTileM,
                  ntiles = ((int64_t)in.N + kJitTileCols - 1) / kJitTileCols;
    const bool long_map = in.K >= 8192 && density > 0.1875 && ntiles > 4 && mtiles > 8;
    return long_map && 4.0 * (double)M * (double)in.K >= kFarXtBytes && 8.0 * nnz <= kFarCodeBytes;
}

// The 64-row image can stage its pieces straight from row-major X (PR rows x
// 1024 / PR contiguous bytes each; tsg_internal.h) when rows start 16-B
// aligned (X 16-B aligned, K % 4 == 0), no piece straddles K (K % (256 / PR)
// == 0: pieces at or past K are omitted, so nothing reads past a row's end)
// and the per-lane offsets fit 32 bits.  Every workgroup of an M tile then
// gathers the same rows, 4K bytes apart, chunk after chunk: that costs more
// than the X^T pass unless a step's work is long enough to hide it -- so
// automatic only for streams of >= 32 adds per k row per wave (width x
// density: 128 columns at s <= 4, 64 at s <= 2).  Measured (kernel / step
// us): configs[2] on 128 x 8 1231.4 / 1239.4 direct vs 1230.4 / 1273.0 staged
// (profiles/r04z_direct_big_ab.jsonl); but s = 16 on 128 x 8 530.7 / 539.5 vs
// 463.3 / 505.8, configs[1] on 16 x 8 94.3 / 101.0 vs 68.5 / 84.3, and K =
// 4096, N = 16384: M = 64 (16 x 4) 85.2-85.7 / 91.6-92.4 vs 65.5-65.9 /
// 78.9-79.5, M = 512 (64 x 8, s = 4) 208-209 / 215 vs 202-205 / 217-220
// (r04f_shape_ab.jsonl, r04g_bound_ab.jsonl).  TSG_JIT_XDIRECT=1 / 0 forces it
// on (where possible) / off, read per call (A/B).
// Row layout (round 5, tsg_internal.h kJit64RowFlag): its pieces read runs of
// contiguous row bytes, as fast from X as from the staged copy
// (profiles/r05_dma_stride_micro.txt), so every call that can reads X
// directly (K >= 188, K % 4 == 0, X 16-B aligned): no X^T pass, no work
// buffer.  The blocked layout keeps the round-4 rule above.
bool x_direct_auto(const PlanInput &in, int nw, int piece_rows)
{
    if (piece_rows == 0) return true;
    const double density = (double)in.nnz / std::max(1.0, (double)in.K * (double)in.N);
    return (double)nw * density >= kXDirectMinAddsPerRow;
}

// K (and X) allow direct X for a 64-row image with this piece shape
bool x_direct_shape_ok(int K, int piece_rows)
{
    return piece_rows == 0 ? K >= kJit64RowChunk && K % 4 == 0 : K > 0 && K % (256 / piece_rows) == 0;
}

// the dispatcher's per-lane X offsets are 32-bit
bool x_direct_offsets_ok(int M, int K) { return (int64_t)M * K * 4 + 4096 < ((int64_t)1 << 32); }

JitShape pick_jit_shape(const PlanInput &in, int M, bool r64 = false);

// The 64-row image (VOP2 adds, one M row per lane) or the 128-row one
// (v_pk_add_f32, two rows per lane) for a call with M rows (that the small-M
// walk does not take); BlockedTCSC runs the 128-row image only.  Measured
// (profiles/r04f_shape_ab.jsonl, r04g_bound_ab.jsonl, r04h_big_ab.jsonl; step
// us, X staged for both): the 64-row image wins at every M <= 512 (K = 4096,
// N = 16384: M = 64 79 vs 121, M = 192 130 vs 163, M = 512 217 vs 243;
// configs[1] 108 vs 116) and above that wherever the 128-row image's shape is
// narrower than 64 x 8 or leaves a round partly empty (N = 16384: M = 640 336
// vs 385, M = 1536 547 vs 617; N = 8192, M = 1024 204 vs 236; N = 4096, M =
// 2048 224 vs 245; K = 16384, N = 4096, M = 2048 806 vs 973); the 128-row
// image keeps the calls its widest shape fills in whole rounds (configs[2]
// 1360 vs 1437, N = 16384 M = 1024 339 vs 358, N = 8192 M = 4096 686 vs 708,
// s = 8 / 16 862 / 637 vs 880 / 661) -- against its 64-wide streams.  At 128
// columns per wave (round 4, profiles/r04l_w128_ab.jsonl, kernel / step us)
// the 64-row image wins those too wherever that shape is its modelled best:
// configs[2] 1286 / 1329 vs 1350 / 1387, s = 8 748 / 790 vs 841 / 886, s = 16
// 500 / 542 vs 609 / 651, N = 16384 M = 1024 320 / 337 vs 331 / 347, M =
// 2048 643 / 664 vs 660 / 685, N = 8192 M = 4096 623 vs 655, configs[2] s = 2
// 2403 vs 2465, (16000, 8192, 2048) 1219 vs 1302, (8192, 16384, 4096) 2467
// vs 2833, (64000, 16384, 4096) s = 8 / 16 11.2 / 7.2 vs 14.3 / 8.7 ms (one
// loss: M = N = K = 4096 361 vs 353); the far-X^T image and dense W over
// long K stay 128-row.
// tcsc_hip_set_tile_rows pins one; TSG_JIT_ROWS64_MAXM replaces the rule by
// M <= its value (A/B).
bool pick_rows64(const PlanInput &in, int M)
{
    static const int env_max = [] {
        const char *e = knob_value("TSG_JIT_ROWS64_MAXM");
        return e ? atoi(e) : -1;
    }();
    if (in.B || !in.jit) return false;
    if (in.tile_rows) return in.tile_rows == 64;
    if (in.jit_force == kJit64WideNW) return true;  // only the 64-row image has that width
    if (env_max >= 0) return M <= env_max;
    if (M <= kRows64AutoMaxM) return true;
    const JitShape s = pick_jit_shape(in, M, false);
    // Round 4 kept two regimes on the 128-row image: the far-X^T image where
    // X^T is >= 8x the Infinity Cache ((64000, 16384, 4096) s = 4 22.1 vs 24.3
    // ms) and dense W over long K ((64000, 16384, 4096) s = 2 39.0 vs 50.6,
    // profiles/r04p_far_ab.jsonl, r04m_w128_big.jsonl).  Round 5's 64-row
    // image reads X directly and takes the long-stream map there too
    // (pick_jit_map), and wins both (step ms, each image in its own process,
    // r05z_longk_maps_ab.jsonl, r05z_longk_maps2_ab.jsonl): (64000, 16384,
    // 4096) s = 4 18.87-19.00 vs 23.37-23.93, s = 2 37.99 vs 39.57; (32000,
    // ...) s = 4 9.40-9.49 vs 12.05-12.15; (8192, ...) s = 2 4.76 vs 4.94.
    const double density = (double)in.nnz / std::max(1.0, (double)in.K * (double)in.N);
    // 128 columns per wave fill whole rounds: twice the adds per staged chunk
    // and per X read of either 64-wide stream (profiles/r04l_w128_ab.jsonl,
    // r04m_w128_big.jsonl) -- for sparse W or long K, and for dense W over
    // short K when its stream reads X directly (x_direct): there the kernels
    // depend on the data (r04o_xdata_ab.jsonl, kernel us: with bench.py's
    // small-integer X the 128-row image runs configs[2] in 1197 vs 1232, with
    // full-mantissa X 1277 vs 1252 -- v_pk_add_f32 slows on high-entropy data,
    // the VOP2 stream hardly), and the 64-row image's step saves the X^T pass:
    // configs[2] 1239.4 vs 1248.8 us per step with integer X
    // (r04z_direct_big_ab.jsonl); the sparse end is the 64-row image's either
    // way (s = 16: 468 vs 569 int, 496 vs 600 frac).
    // x_direct's own limits that M and K decide (the 32-bit per-lane offsets:
    // X below 4 GiB); X's alignment is checked per call
    const bool direct_capable = x_direct_shape_ok(in.K, jit64_piece_rows()) &&
                                x_direct_auto(in, kJit64WideNW, jit64_piece_rows()) &&
                                x_direct_offsets_ok(M, in.K);
    // round 5: whenever the 64-row image reads X directly (the row layout: K
    // >= 188, K % 4 == 0) its call is one launch, while the 128-row image's
    // step adds its X^T pass -- the 128-row image's whole-round shapes below
    // lose their step too (r05z_n512_ab.jsonl, step us, M = 64000, N = 512:
    // K = 4096 s = 4 693 vs 1093, K = 16384 2690 vs 4244, K = 1024 s = 16 170
    // vs 261)
    if (direct_capable) return true;
    // X past the 32-bit offsets: both images stage X, as in round
    // 4, whose two rules for that regime stand -- the far-X^T image (128-row
    // only) where X^T is >= 6x the Infinity Cache ((64000, 16384, 4096) 22.1
    // vs 24.3 ms for the 64-row 128 x 8, profiles/r04p_far_ab.jsonl), and the
    // 128-row long-stream map for dense W over long K with few columns
    // ((64000, 16384, 4096) s = 2 39.0 vs 50.6 ms, r04m_w128_big.jsonl)
    if (x_direct_shape_ok(in.K, jit64_piece_rows()) && !x_direct_offsets_ok(M, in.K)) {
        if (s.far && 4.0 * (double)M * (double)in.K >= kFarKeepXtBytes) return false;
        if (in.K >= 16384 && in.N <= 8192 && density > 0.375) return false;
    }
    if ((density <= 0.1875 || in.K >= 8192) && pick_jit_shape(in, M, true).nw == kJit64WideNW) return true;
    if (s.nw != kJitNW || s.waves != kJitWaves) return true;
    const int64_t wgs = (int64_t)((M + kJitTileM - 1) / kJitTileM) *
                        ((in.N + (int64_t)s.waves * s.nw - 1) / ((int64_t)s.waves * s.nw));
    const int64_t rounds = (wgs + kJitOneRoundWgs - 1) / kJitOneRoundWgs;
    return (double)wgs < kRows64FullRound * (double)(rounds * kJitOneRoundWgs);
}

JitShape pick_jit_shape(const PlanInput &in, int M, bool r64)
{
    static const int env_waves = [] {
        const char *e = knob_value("TSG_JIT_WAVES");
        return e ? atoi(e) : 0;
    }();
    if (in.B) return {kJitNW, kJitWaves};
    // the 64-row image's half ring for its 4-wave shapes (TSG_JIT_HALF=1, read per call: A/B)
    const char *hv = r64 ? knob_value("TSG_JIT_HALF") : nullptr;
    const bool half_on = hv && hv[0] == '1';
    if (in.jit_force) {
        const int f = !r64 && in.jit_force == kJit64WideNW ? kJitNW : in.jit_force;
        const int w = env_waves == 4 && jit_waves_ok(f, 4) ? 4 : kJitWaves;
        return {f, w, !r64 && f == kJitNW && w == kJitWaves && far_xt(in, M), r64, r64 && w == 4 && half_on};
    }
    const int tile_m = r64 ? kJit64TileM : kJitTileM;
    const int64_t mt = (std::max(M, 1) + tile_m - 1) / tile_m;
    const double image8 = (r64 ? 4.0 : 8.0) * (double)in.nnz;
    if (r64) {
        // 64-row image: the shape with the least modelled time = rounds of
        // one-workgroup-per-CU x the time of a workgroup, which grows with the
        // columns a SIMD carries (width x waves / 4) scaled by density, over a
        // fixed part (the K sweep's staging and barriers).  A lone wave per
        // SIMD (4-wave workgroups) issues its VOP2 adds at half the rate of a
        // pair, and 8-column streams feed few adds per X read.  Fitted on
        // one-round grids at K = 4096, s = 4 with X staged
        // (profiles/r04j_waves_ab.jsonl, kernel us): configs[1] 16 x 8 79.6 vs
        // 32 x 4 92.8; M = 128, N = 16384: 16 x 8 87.1 vs 32 x 4 91.3-96.7;
        // M = 64: 16 x 4 66.2 vs 8 x 8 76.0; M = 256, N = 4096: 16 x 4
        // 56.1-58.9 vs 8 x 8 59.3.  A fractional round costs a whole one
        // (M = 192: 32 x 4 on 384 workgroups 178 us; one round of 32 x 8 123).
        // Ties go to the wider stream (fewer LDS reads per add).
        const double dens4 = 4.0 * (double)in.nnz / std::max(1.0, (double)in.K * (double)in.N);
        JitShape pick{kJitNW, kJitWaves, false, true};
        double best_cost = 0.0;
        bool any = false;
        for (int nw : kJit64Widths)
            for (int waves : {kJitWaves, 4}) {
                if (!jit_waves_ok(nw, waves)) continue;
                if (env_waves == 4 && nw < kJitNW && waves != 4) continue;
                const int64_t ntile = (in.N + (int64_t)waves * nw - 1) / ((int64_t)waves * nw), wgs = mt * ntile;
                const double image = image8 + (double)ntile * waves * in.jit_nch * 2 * (160.0 + 8.0 * kJitChunk);
                if (nw != kJitNW && image > 2.0 * (double)(1ull << 30)) continue;
                const double rounds = (double)((wgs + kJitOneRoundWgs - 1) / kJitOneRoundWgs);
                const double adds = (double)nw * waves / 4.0 * dens4 * (waves == 4 ? 1.35 : 1.0);
                const double cost = rounds * (48.0 + adds + (nw == 8 ? 10.0 : 0.0));
                if (!any || cost < best_cost) {
                    any = true;
                    best_cost = cost;
                    pick = {nw, waves, false, true};
                }
            }
        pick.half = pick.waves == 4 && half_on;
        return pick;
    }
    JitShape best{kJitNW, kJitWaves}, most{kJitNW, kJitWaves};
    int64_t most_wgs = -1;
    bool full = false;
    for (int nw : kJitWidths) {
        for (int waves : {kJitWaves, 4}) {
            if (!jit_waves_ok(nw, waves)) continue;
            if (env_waves == 4 && nw != kJitNW && waves != 4) continue;
            const int64_t ntile = (in.N + (int64_t)waves * nw - 1) / ((int64_t)waves * nw), wgs = mt * ntile;
            // narrow streams repeat the reads and step scaffolding per stream:
            // keep the image inside the 32-bit stream offsets
            const double image = image8 + (double)ntile * waves * in.jit_nch * 2 * (160.0 + 8.0 * kJitChunk);
            if (nw != kJitNW && image > 2.0 * (double)(1ull << 30)) continue;
            if (!full && wgs >= kJitFullWgs) {  // widths come widest first
                best = {nw, waves};
                full = true;
            }
            if (wgs > most_wgs) {
                most_wgs = wgs;
                most = {nw, waves};
            }
        }
    }
    JitShape sh = full ? best : most;
    sh.far = !r64 && sh.nw == kJitNW && sh.waves == kJitWaves && far_xt(in, M);
    sh.r64 = r64;
    return sh;
}

// The generated code's per-group code touches (tsg_jit.cpp, round 6: a 128-
// wide dense stream writes more code per step than the step's one 8-KiB
// touch covers) run where they were measured to pay: X of at most 384 MiB
// (~1.5x the Infinity Cache), and dense W (s <= 2: steps of ~25 KiB of code)
// with X up to 1 GiB.  With large X they cost more than they save
// (profiles/r06h_tgroup_longk_ab.jsonl, kernel us: (16000, 16384, 4096) s = 4
// 5221 vs 4727 off, (16000, 8192, 2048) s = 4 1371 vs 1203;
// r06i_xtouch_big_ab.jsonl: (64000, 16384, 4096) s = 2 34.2-46.5 ms, unsteady,
// vs 38.0-38.4 off) -- but (4096, 16384, 4096) 1115 vs 1192, configs[2] 1157
// vs 1221, (16000, 8192, 2048) s = 2 2152 vs 2394.  Elsewhere the dispatcher
// points them all at one line.  TSG_JIT_XTOUCH=0|1 forces it (A/B, per call).
bool pick_xtouch(const PlanInput &in, int M)
{
    if (const char *e = knob_value("TSG_JIT_XTOUCH")) return e[0] == '1';
    const double density = (double)in.nnz / std::max(1.0, (double)in.K * (double)in.N);
    const double xbytes = 4.0 * (double)M * (double)in.K;
    return xbytes <= kXTouchMaxXBytes || (density > 0.375 && xbytes <= kXTouchDenseMaxXBytes);
}

// The code-touch window (tsg_jit.cpp: 8 KiB, from 8 KiB ahead of the step's
// position) starts at the step's own position instead -- the dispatcher
// moves the touch base back 8 KiB -- for 64-row calls with at most 2 M
// tiles, and on 4-wave workgroups: with few M tiles each code line is
// fetched by few workgroups, much of it straight from HBM, and the nearer
// window pays (profiles/r06j_touch_small_ab.jsonl, r06p_touch_8w_ab.jsonl,
// kernel us: M = 64 / 48, N = 16384 (16 x 4) 58.9 / 57.4 -> 51.7 / 50.0,
// M = 128 (16 x 8, 2 M tiles) 74.3 -> 64.4, (64, 2048, 8192) s = 2 32.1 ->
// 28.6, (1024, 4096, 1024) (16 x 4) 56.1 -> 54.9; M = 192 (3 tiles) -1%,
// configs[1] (8 tiles) +1%, (256, 4096, 8192) a tie).  TSG_JIT_TNEAR=0|1
// forces it (A/B, read per call).
bool pick_tnear(bool r64, int waves, int mtiles)
{
    if (const char *e = knob_value("TSG_JIT_TNEAR")) return e[0] == '1';
    return r64 && (mtiles <= 2 || waves == 4);
}

// The image and shape a jit call with M rows runs: the automatic (or pinned)
// pick, unless that image failed to load at an earlier call -- then the
// 128-row 64 x 8 image (run_dev's fallback, which loads it).
JitShape call_shape(const PlanInput &in, int M)
{
    const JitShape sh = pick_jit_shape(in, M, pick_rows64(in, M));
    if (((in.bad_variants >> variant_bit(sh)) & 1u) && may_fall_back(in, sh)) return JitShape{kJitNW, kJitWaves};
    return sh;
}

// Tile map groups (tsg_jit_map.h) per call: gn column tiles x gm M tiles per
// XCD group, 32 workgroups (the XCD's CUs).  Measured
// (profiles/r03_map_density_ab.txt, r02_jit_map_bench_ab.txt):
//  * with at most 4 column tiles or 8 M tiles, 4 x 8: every column tile, or
//    every M tile, of the XCD's group shares its X^T chunks or code
//    ((16000, 8192, 2048) 1.19-1.21 vs 1.31-1.34 ms at 2 x 16);
//  * sparse W (density <= 3/16, s >= 8): 4 x 8 -- a column tile's code is
//    short, so sharing each X^T slab between more column tiles wins (s = 16:
//    0.565 vs 0.604 ms at 2 x 16; s = 8: 0.769 vs 0.792);
//  * long streams (K >= 8192, density > 3/32): 1 x 32, every CU of the XCD on
//    one column tile's code ((64000, 16384, 4096): 25.6 vs 26.8 ms; s = 8
//    13.7 vs 15.3-15.8 ms);
//  * otherwise 2 x 16: the CU pairs that share an instruction cache on one
//    code stream (configs[2] 1.212 ms vs 1.264 at 4 x 8; s = 2 2.554 vs 2.712).
// Code touches (tsg_jit_kernel.hip): only M tiles with (mt & tmask) == 0
// spread theirs over the stream's lines.  When the whole grid is resident at
// once (<= 256 workgroups: one per CU) and >= 4 M tiles share each stream,
// those M tiles run together, so one touch in four serves them (profiles/
// r03e_touch_ab.txt, r03e_long_k_ab.txt: configs[1] 0.0989-0.1013 -> 0.0931-
// 0.0938 ms, (1024, 4096, 1024) 0.0878 -> 0.0834, (1024, 16384, 1024) 0.317 ->
// 0.303); with several rounds the touching tile may not run beside the others
// (configs[2] +4%, s = 16 +15%), and with 2 M tiles per stream it loses too
// ((256, 4096, 16384) +7-17%, r03g_ref_cases.jsonl), so every tile touches.
// TSG_JIT_GN / TSG_JIT_GM / TSG_JIT_TMASK override (A/B).
void pick_jit_map(const PlanInput &in, int mtiles, int ntiles, int &gn, int &gm, int &tmask, int nw = 0)
{
    static const int env_gn = [] { const char *e = knob_value("TSG_JIT_GN"); return e ? atoi(e) : 0; }();
    static const int env_gm = [] { const char *e = knob_value("TSG_JIT_GM"); return e ? atoi(e) : 0; }();
    static const int env_tm = [] { const char *e = knob_value("TSG_JIT_TMASK"); return e ? atoi(e) : -1; }();
    const double density = (double)in.nnz / std::max(1.0, (double)in.K * (double)in.N);
    // the 64-row image's 128-wide streams thin their touches over several
    // rounds too: configs[2] 1.2243-1.2252 vs 1.2315-1.2317 ms kernel, three
    // alternating bench runs each (profiles/r04t_tmask_bench_ab.txt); configs[3]
    // s = 8 / 16 680.6-681.2 / 444.3-448.1 vs 684.7-690.5 / 458.2-462.8 us
    // (r04t_tmask_sparse_ab.txt); (16000, 8192, 2048) s = 4 / 8 1227-1239 /
    // 729-735 vs 1248-1261 / 739-749 us (r04t_tmask_long_ab.txt; (8192, 16384,
    // 4096) within its run-to-run spread) -- but not for sparse W over long K
    // (round 5, direct X on the row layout, kernel us, r05p_tmask_long_ab.jsonl):
    // (64000, 16384, 4096) s = 8 / 16 14640 / 8310 thinned vs 10796 / 7020
    // with every tile touching, (16000, 8192, 2048) s = 8 / 16 799 / 532 vs
    // 726 / 494; (8192, 16384, 4096) s = 4 a tie (2359 vs 2355)
    const bool wide_short = nw == kJit64WideNW && (in.K < 8192 || density > 0.1875);
    tmask = env_tm >= 0 ? env_tm
                        : (((int64_t)mtiles * ntiles <= kJitOneRoundWgs || wide_short) && mtiles >= 4 ? 3 : 0);
    int n = 2, m = 16;
    // s = 8 over long K takes the long-stream map ((64000, 16384, 4096) s = 8:
    // 13.72-13.73 ms vs 15.3-15.8 at 4 x 8, profiles/r03f_sparse_big_ab.txt);
    // s = 16 stays on 4 x 8 (8.38-8.45 vs 11.66 at 1 x 32)
    const bool long_sparse = in.K >= 8192 && density > 0.09375;
    // round 5: the 64-row image's 128-wide streams over K >= 16384 with dense
    // W (s <= 4) take the long-stream map even on <= 4 column tiles -- an XCD
    // on one tile's code, 32 M tiles in step through it (profiles/
    // r05z_longk_maps_ab.jsonl, step ms, 1 x 32 vs 4 x 8: (64000, 16384,
    // 4096) s = 2 / 4 37.99 / 18.87 vs 50.15 / 24.71, (16000, ...) s = 4 4.73
    // vs 4.94, (8192, ...) s = 2 4.76 vs 4.92, s = 4 and (4096, ...) ties;
    // s = 8 stays 4 x 8: 10.90 vs 12.99; K = 8192, N = 2048 too: 1.19 vs 1.41)
    // (and K = 8192 with >= 4 column tiles: (64000, 8192, 4096) s = 4 10.91 vs
    // 12.86, (32000, 8192, 4096) s = 2 9.08 vs 12.20; with 2 column tiles 4 x 8
    // (gn = 2) stays: (64000, 8192, 2048) a tie, (16000, 8192, 2048) 1.19 vs
    // 1.41; r05z_k8192_maps_ab.jsonl)
    // The 64-row image takes the long-stream map only with >= 64-column
    // streams and >= 32 M tiles (a full group): narrower streams and half
    // groups run faster on 4 x 8 (r05z_midm_longk_maps_ab.jsonl, us, 4 x 8
    // vs 1 x 32 / 1 x 16: (1024, 16384, 4096) 32 x 8 374 vs 471, (2048, 8192,
    // 1024) s = 2 16 x 8 165 vs 210, (1024, 8192, 16384) 128 x 8 600 vs 630;
    // the long map (2048, 16384, 4096) 64 x 8 622 vs 709, (2048, 16384,
    // 16384) s = 2 4929 vs 6014)
    const bool long_ok = nw == 0 || (nw >= 64 && mtiles >= 32);
    const bool long_dense_wide = nw == kJit64WideNW && in.K >= 8192 && density > 0.1875 && mtiles >= 32 &&
                                 (in.K >= 16384 || ntiles >= 4);
    if (!long_dense_wide && (ntiles <= 4 || mtiles <= 8 || (density <= 0.1875 && !long_sparse))) {
        n = 4;
        m = 8;
    } else if (in.K >= 8192) {
        n = long_dense_wide || long_ok ? 1 : 4;
        m = long_dense_wide || long_ok ? 32 : 8;
    }
    gn = std::min(env_gn > 0 ? env_gn : n, std::max(ntiles, 1));  // a group never exceeds the grid
    gm = std::min(env_gm > 0 ? env_gm : m, std::max(mtiles, 1));
}

// The producer/consumer walk (tsg_tcsc_ell_pc_kernel) on 1-row tiles when K
// fits one chunk and the chunk plus its ring fit LDS: few chains, each
// latency-bound (M = 1: 15.6 vs 20.6 us at K = 4096, N = 16384;
// profiles/r02x_ell_pc.txt).  TSG_ELL_PC=0 turns it off (diagnostic A/B);
// tcsc_hip_set_small_m(h, 3) too.
bool ell_pc_available(const PlanInput &in)
{
    static const bool on = [] {
        const char *e = knob_value("TSG_ELL_PC");
        return !(e && e[0] == '0');
    }();
    if (!on || in.small_m == 3 || in.K > kEllMaxC[0]) return false;
    const int C = std::min(kEllMaxC[0], std::max(4, (in.K + 3) / 4 * 4));  // build_ell_image's chunk
    const size_t lds = ell_pc_lds_bytes(0, C);
    return lds > 0 && lds <= kLdsBytes;
}

bool use_ell_pc(const PlanInput &in, int v) { return v == 0 && ell_pc_available(in); }

// Small-M kernel choice (DESIGN.md 4 "Small M"): the sliced-ELL walk for a
// plain-TCSC weight-compiled handle when M is small enough that the jit
// kernel cannot fill the GPU; -1 = the jit (or rx) kernel.  Measured on
// configs[2]'s and configs[0]'s K, N (profiles/r02u_ell_lg.txt): up to M = 8
// the smallest M tile that holds M; up to M = 32 tiles of 8 (2 rows per lane:
// an 8-row chunk of K <= 5116 fits LDS, one stream per column); above that the
// largest tile whose chunk holds K.  Automatic (round 4, against the 64-row
// image, profiles/r04g_bound_ab.jsonl, step us) up to M = 32 while an 8-row
// chunk holds K (K = 4096, N = 16384: M = 32 56 vs 70, M = 48 101 vs 71), up to
// M = 16 when K is chunked (K = N = 16384: M = 16 184 vs 247, M = 32 310 vs
// 248; K = 16384, N = 4096: M = 16 178 vs 158, M = 32 281 vs 155); and, while
// an 8-row chunk holds K, up to M = 1024 when the jit kernel would have at
// most 64 workgroups (the reference's (1000, 2048, 512): 38 vs 52 us;
// (256, 4096, 1024): 41 vs 82; (256, 2048, 2048): 37 vs 47; at 128 workgroups
// the jit kernel wins: (1024, 1024, 1024) 43 vs 35).  With K chunked the
// starved grid goes to the 64-row image ((64, 16384, 4096): 266 vs 156 us).
int pick_ell_variant(const PlanInput &in, int M)
{
    if (!in.jit || in.B || in.small_m == 1) return -1;
    const bool one8 = in.K <= kEllMaxC[kEllTile8];
    // the jit kernel's workgroups at its narrowest width (8 columns per wave)
    const int64_t jit_wgs = (int64_t)((M + kJitTileM - 1) / kJitTileM) *
                            ((in.N + 8 * kJitWaves - 1) / (8 * kJitWaves));
    const bool starved = one8 && M <= kEllStarvedMaxM && jit_wgs <= kEllStarvedWgs;
    static const int env_max = [] {  // TSG_ELL_MAXM: A/B of the small-M boundary (not of the small-W rule)
        const char *e = knob_value("TSG_ELL_MAXM");
        return e ? atoi(e) : -1;
    }();
    const int auto_max = env_max >= 0 ? env_max : kEllAutoMaxM;
    // a small W (M x nnz <= 420 M) keeps the walk up to M = 128 while K fits
    // one chunk: the 64-row image streams its whole code image and stages X
    // (~13 us of step overhead against ~6) whatever M is, the walk's cost
    // grows with M x nnz (profiles/r04r_sparse_small_ab.jsonl, step us:
    // (64, 2048, 8192) s = 8 26.6 vs 36.9, s = 16 21.7 vs 35.2, s = 4 35.9 vs
    // 41.0; (96, 4096, 16384) s = 16 61.3 vs 77.9; beyond it the image wins:
    // (128, 4096, 16384) s = 16 80.3 vs 76.1, (64, 4096, 16384) s = 8 66.2 vs
    // 63.0, s = 4 at M = 48 101 vs 71)
    const bool small_w = one8 && M <= kEllSmallWMaxM && (double)M * (double)in.nnz <= kEllSmallWWork;
    // ... unless the 64-row image (one launch, X read directly since round 5)
    // is faster there even at its floor: its K sweep costs ~0.9 us per step (2
    // passes over ceil(K / 188) chunks) + 1.4, the walk's chains ~9.9 +
    // 0.0143 us per entry of a column (K / s); profiles/r05z_walk_vs_image2.jsonl
    // (88 shapes with r05z_walk_vs_image_ab.jsonl: the round-4 rule picked the
    // slower kernel by > 3% on 21, this one on 4), step us: K = 1024, s = 4, M = 48 ... 1024, N = 512 / 1024 /
    // 4096 12.2-15.6 vs 13.6-18.8 (every M); s = 16 10.8-11.1 walk vs
    // 11.6-12.2; K = 2048 walk 17.2 vs 19.5 (M <= 256)
    // (this floor was measured with X read directly, one launch: with K % 4 !=
    // 0 or X past the 32-bit offsets the image's step also runs its X^T
    // staging kernel, priced here at kStagedXtUs -- ADVICE r05)
    const bool image_one_launch = x_direct_shape_ok(in.K, jit64_piece_rows()) && x_direct_offsets_ok(M, in.K);
    const double nnz_col = (double)in.nnz / std::max(1, in.N);
    const bool image_floor_lower = 0.9 * 2.0 * ((in.K + kJit64RowChunk - 1) / kJit64RowChunk) + 1.4 +
                                       (image_one_launch ? 0.0 : kStagedXtUs) <
                                   9.9 + 0.0143 * nnz_col;
    if (in.small_m < 2 && M > (one8 ? auto_max : std::min(auto_max, kEllAutoMaxMChunked)) &&
        ((!starved && !small_w) || image_floor_lower))
        return -1;
    // K in chunks (the 16-row tile, 8 columns per wave) at 8 < M <= 16: the
    // walk needs >= 2048 waves (N >= 16384) to beat the 64-row image
    // (r05z_walk_longk2_ab.jsonl, us, image vs walk: (16, 8192, 8192) 81.6 vs
    // 96.4, (12, 8192, 4096) 68.7 vs 91.3, (16, 16384, 4096) 131.7 vs 181.0,
    // (16, 8192, 2048) 66.3 vs 96.2; the walk (16, 16384, 16384) 170 vs 205,
    // and at M <= 8 (8, 8192, 4096) 61.5 vs 68.5, r05z_walk_longk_ab.jsonl)
    // (measured with direct X; the image's margin, 15-50 us, exceeds its X^T
    // pass at these M -- 16 x 8194 floats -- so the rule holds staged too)
    if (in.small_m < 2 && !one8 && M > 8 && in.N < 16384) return -1;
    int v = 0;
    if (one8 && M > kEllTileM[kEllTile8] && M <= kEllMidM) {
        v = kEllTile8;
    } else if (one8 && M > kEllMidM) {
        v = kEllTile8;
        for (int i = kEllTile8 + 1; i < kEllVariants; i++)
            if (in.K <= kEllMaxC[i]) v = i;
    } else {
        while (v + 1 < kEllVariants && M > kEllTileM[v]) v++;
    }
    // M rows as M 1-row producer/consumer tiles while the M index streams stay
    // small (M = 2 at N = 16384: 20.0 vs 22.9 us; M = 4 at N = 4096: 14.7 vs
    // 21.9 us; profiles/r02z2_pc_rows.txt)
    static const int64_t pc_rows_max_mn = [] {  // TSG_ELL_PC_MAXMN: A/B sweeps of the threshold
        const char *e = knob_value("TSG_ELL_PC_MAXMN");
        return e ? (int64_t)atoll(e) : kEllPcRowsMaxMN;
    }();
    if (M <= 4 && (int64_t)M * in.N <= pc_rows_max_mn && ell_pc_available(in)) v = 0;
    static const int force = [] {  // TSG_ELL_VARIANT: diagnostic sweeps only
        const char *e = knob_value("TSG_ELL_VARIANT");
        return e ? atoi(e) : -1;
    }();
    if (force >= 0 && force < kEllVariants) v = force;
    return v;
}

}  // namespace

int width_index(int nw)
{
    for (int i = 0; i < 4; i++)
        if (kJitWidths[i] == nw) return i;
    return -1;
}

// jv index of a (width, waves) shape: 8-wave widths 0..3, 4-wave widths
// 32/16/8 4..6, the 64 x 8 far-X^T image 7; jv64 (the 64-row image): the
// same 0..6 and 128 x 8 at 7
int shape_index(int nw, int waves, bool far)
{
    if (nw == kJit64WideNW) return waves == kJitWaves && !far ? 7 : -1;
    const int w = width_index(nw);
    if (w < 0 || !jit_waves_ok(nw, waves) || (far && (nw != kJitNW || waves != kJitWaves))) return -1;
    return far ? 7 : waves == kJitWaves ? w : 3 + w;
}

int shape_index(const JitShape &sh) { return shape_index(sh.nw, sh.waves, sh.far && !sh.r64); }

// bit of a shape in PlanInput::bad_variants: 128-row 0..7, 64-row 8..15, half ring 16..18
int variant_bit(const JitShape &sh)
{
    return sh.r64 && sh.half ? 16 + width_index(sh.nw) - 1 : (sh.r64 ? 8 : 0) + shape_index(sh);
}

bool x_direct(const PlanInput &in, const JitShape &sh, int piece_rows, bool x_aligned, int M)
{
    if (!sh.r64) return false;
    // the layout of an image not built yet: the half ring has no row layout
    if (piece_rows < 0)
        piece_rows = sh.half ? (jit64_piece_rows() ? jit64_piece_rows() : 16) : jit64_piece_rows();
    const char *e = knob_value("TSG_JIT_XDIRECT");
    const bool on = e ? e[0] == '1' : x_direct_auto(in, sh.nw, piece_rows);
    return on && x_direct_shape_ok(in.K, piece_rows) && x_aligned && x_direct_offsets_ok(M, in.K);
}

int64_t jit_tiles(int M, int N, int tile_m, int cols)
{
    return (int64_t)((std::max(M, 1) + tile_m - 1) / tile_m) * ((N + cols - 1) / cols);
}

// Not automatic: no call loops unless TSG_JIT_LOOP names a grid (DESIGN.md
// 4.2 has the A/B that decides this, profiles/loop_ab.jsonl).
int loop_wgs(const JitShape &sh, int64_t tiles)
{
    if (!sh.r64 || sh.half || sh.waves != kJitWaves) return 0;
    const char *e = knob_value("TSG_JIT_LOOP");
    const int g = e ? atoi(e) : 0;  // 0: never; else the grid as given
    return g > 0 && tiles > g ? g : 0;
}

// A call may fall back from an image that cannot be loaded to the 128-row
// 64 x 8 image when nothing pinned its image or shape (a pinned request fails
// loudly instead: TSG_ERR_HIP).
bool may_fall_back(const PlanInput &in, const JitShape &sh)
{
    const bool is_default = !sh.r64 && !sh.far && sh.nw == kJitNW && sh.waves == kJitWaves;
    return !is_default && !in.tile_rows && !in.jit_force && in.far_mode != 2 &&
           !knob_value("TSG_JIT_ROWS64_MAXM") && !knob_value("TSG_JIT_NW");
}

// What a call with M rows runs.  The map and the touch settings need only
// the shape: an image's column tiles are ceil(N / (width x waves)) by
// construction (tsg_jit.cpp build_jit_code), so the plan exists before the
// image does.
CallPlan plan_call(const PlanInput &in, int M)
{
    CallPlan p;
    p.xtouch = pick_xtouch(in, M) ? 1 : 0;
    p.ell = pick_ell_variant(in, M);
    if (p.ell >= 0) {
        // small M: the ELL walk reads X in place (no X^T staging, no work buffer)
        p.kernel = use_ell_pc(in, p.ell) ? Kernel::kEllPc : Kernel::kEll;
        return p;
    }
    if (!in.jit) {
        p.kernel = Kernel::kRx;
        p.tile_m = kRxTileM;
        p.chunk = kRxChunk;
        return p;
    }
    const JitShape sh = p.shape = call_shape(in, M);
    p.kernel = sh.r64 ? Kernel::kJit64 : Kernel::kJit128;
    p.tile_m = sh.r64 ? kJit64TileM : kJitTileM;
    p.chunk = sh.r64 ? jit64_chunk(sh.half) : kJitChunk;
    const int cols = sh.nw * sh.waves;
    const int mtiles = (std::max(M, 1) + p.tile_m - 1) / p.tile_m, ntiles = (in.N + cols - 1) / cols;
    pick_jit_map(in, mtiles, ntiles, p.gn, p.gm, p.tmask, sh.r64 ? sh.nw : 0);
    p.tnear = pick_tnear(sh.r64, sh.waves, mtiles) ? 1 : 0;
    return p;
}

// Chunks of the host-pointer pipeline: one per ~16 MiB of Y (the PCIe leg
// that binds: Y is the largest transfer), at most kHostChunksMax, each a whole
// number of 128-row M tiles and at least 256 rows; calls the small-M kernel
// takes run whole.  configs[2] (268 MB of Y): 16 chunks of 256 rows, 5.45 ms
// per call (8 chunks 5.50, 4 chunks 5.72, unchunked 7.38;
// profiles/r03b_host_pipe_ab.jsonl).
int host_chunk_rows(const PlanInput &in, int host_chunks, int M)
{
    const int64_t ybytes = (int64_t)M * in.N * 4;
    int n = host_chunks > 0 ? host_chunks : (int)std::min<int64_t>(ybytes >> 24, kHostChunksMax);
    n = std::min(n, kHostChunksMax);
    if (n <= 1 || (host_chunks <= 0 && pick_ell_variant(in, M) >= 0)) return M;
    int rows = (M + n - 1) / n;
    rows = (rows + kJitTileM - 1) / kJitTileM * kJitTileM;
    if (host_chunks <= 0) rows = std::max(rows, 256);
    return std::min(rows, M);
}

}  // namespace tsg
