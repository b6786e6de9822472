// tsg_capi.cpp -- the HIP runtime side of the C-ABI (include/ternary_spgemm.h):
// handle lifetime, device image upload, work buffer, streams and events, the
// launches of each kernel family, the host-pointer pipeline.  What a call
// runs is decided by the planner (tsg_plan.h); no policy lives here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <iterator>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ternary_spgemm_test.h"
#include "tsg_internal.h"
#include "tsg_plan.h"

using tsg::CallPlan;
using tsg::JitShape;
using tsg::Kernel;

extern thread_local std::string g_tsg_host_err;  // one per-thread message for the whole ABI

static int fail(int code, const std::string &msg)
{
    g_tsg_host_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(TSG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

struct tsg_tcsc {
    // everything the planner reads: K, N, B, nnz, the kernel family (jit:
    // weight-compiled, default; else rx, the register-X walk: images too large
    // for 32-bit stream offsets, a failed image load, or TSG_KERNEL=rx), the
    // pins the setters write and the images that failed to load
    tsg::PlanInput plan;
    int device = 0;
    int cus = 0;                          // its compute units, read once at registration (TSG_JIT_DIAG=onetile)
    int last_grid = 0, last_tiles = 0;    // workgroups and logical ids of the last weight-compiled launch (test hook)
    int64_t nnz_pos = 0, nnz_neg = 0;
    tsg::RxImage rimg;                    // device image of the rx kernel
    // jit kernel: one compiled image per (stream width, waves per workgroup)
    // (shape_index): the default shape at registration, others on the first
    // call with an M that picks them (or tcsc_hip_reserve)
    struct JitVariant {
        int nw = 0, waves = 0, Npad = 0;
        int piece_rows = 0;               // 64-row image: rows per DMA piece (its X^T layout; 0 = row layout)
        bool pair = false;                // 64-row 4-wave streams run by 8-wave workgroups of wave pairs
        int nch = 0, chunk = 0;           // X^T chunks of the image and K rows per chunk
        tsg::JitModule mod;               // dispatcher + generated code, loaded
        uint32_t *d_wcode = nullptr;      // per (column tile, stream): byte offset of its code
        int64_t code_bytes = 0, wcode_words = 0;
    };
    JitVariant jv[8];                     // 7: the 64 x 8 "far X^T" image (tsg_plan.cpp pick_jit_shape)
    JitVariant jv64[8];                   // the 64-row image (tsg_internal.h), shape_index 0..7
    JitVariant jv64h[3];                  // its half ring (kJit64HalfChunk): 4-wave widths 32, 16, 8
    uint32_t *d_status = nullptr;         // jit dispatcher status word (nonzero: region check failed)
    // small-M kernel (tsg_ell.hip): one sliced-ELL image per variant, built on
    // the first call (or tcsc_hip_reserve) that picks the variant
    struct EllVariant {
        tsg::EllImage img;                // host metadata (C, nch, ...); arrays freed after upload
        uint32_t *d_ent = nullptr, *d_tab = nullptr;
        int64_t bytes = 0;
        bool ready = false;
    };
    EllVariant ell[tsg::kEllVariants];
    std::vector<int32_t> csp, csn, rip, rin;  // host TCSC (getVectorRepresentation)
    uint32_t *d_seg = nullptr, *d_ent = nullptr;
    float *d_work = nullptr;              // X^T [Kp][Mp]
    size_t work_bytes = 0;
    // d_work is shared by every call on the handle: the last stream that read
    // it and an event recorded after that read; a call on another stream
    // waits for the event before it overwrites X^T (run_dev)
    hipStream_t work_stream = nullptr;
    hipEvent_t work_ev = nullptr;
    bool work_used = false;
    // scratch of the actquant and normquant calls (tsg_actquant.h, tsg_norm.h):
    // inv at d_aq[0, aq_rows), deq at d_aq[aq_rows, 2 aq_rows), the rn of a
    // normquant call at d_aq[2 aq_rows, 3 aq_rows), and the int8 q (M x K) of a call that
    // runs a small-M walk.  Grow-only and shared by every stream like d_work:
    // the same event orders its reuse (work_begin / work_end)
    float *d_aq = nullptr;
    size_t aq_rows = 0;
    int8_t *d_aq8 = nullptr;
    size_t aq8_bytes = 0;
    // host-pointer path staging (tcsc_hip_gemm): grow-only
    float *d_x = nullptr, *d_b = nullptr, *d_y = nullptr, *d_alpha = nullptr;
    size_t x_bytes = 0, y_bytes = 0;
    hipStream_t stream = nullptr;         // stream of the host-pointer path (compute)
    std::mutex host_mu;                   // one host-pointer call at a time (its staging buffers)
    // host-pointer pipeline (run_host): X chunks in on s_in, chunk compute on
    // `stream`, Y chunks out on s_out; one event pair per chunk
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[tsg::kHostChunksMax] = {}, ev_c[tsg::kHostChunksMax] = {};
    int host_chunks = 0;                  // tcsc_hip_set_host_chunks: 0 = automatic
    // timing of the main kernel
    bool timing = false;
    static constexpr int kRing = 256;     // event pairs in flight before a harvest blocks
    hipEvent_t ev0[kRing] = {}, ev1[kRing] = {};
    int ring_head = 0, ring_count = 0;    // pending pairs: [head - count, head)
    double total_ms = 0.0;
    int64_t launches = 0;
    // run_dev, reserve and the setters write the plan state (plan, JitVariant)
    // under it; the const per-call queries read under it too
    mutable std::mutex mu;
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int check_device(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(TSG_ERR_NODEV, "hipGetDeviceProperties failed for device " + std::to_string(dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TSG_ERR_NODEV, std::string("device is ") + prop.gcnArchName +
                                       "; this library is built for gfx950 (MI355X) only");
    return TSG_OK;
}

// X^T dimensions of a call with M rows: rows padded to the M tile, K to
// whole chunks (every image has max(1, ceil(K / chunk)) chunks; 64-row image:
// k-quad layout, 64-row tiles, 192-row chunks)
struct XtDims {
    int Mp, Kp;
};
XtDims dims_for(int M, int K, int tile_m, int chunk)
{
    return {((std::max(M, 1) + tile_m - 1) / tile_m) * tile_m, std::max(1, (K + chunk - 1) / chunk) * chunk};
}

// Grows the X^T work buffer (grow-only).  A grow frees the old buffer, so it
// first waits for every launch that may still read it; it cannot happen while
// a stream is being captured (tcsc_hip_reserve(max_M) before the capture).
int ensure_work(tsg_tcsc *h, int M, int tile_m, int chunk, bool capturing)
{
    const XtDims d = dims_for(M, h->plan.K, tile_m, chunk);
    const size_t need = (size_t)d.Mp * d.Kp * sizeof(float);
    if (need <= h->work_bytes) return TSG_OK;
    if (capturing)
        return fail(TSG_ERR_ARG, "M=" + std::to_string(M) + " needs a larger work buffer during stream capture; "
                                 "call tcsc_hip_reserve(h, max_M) before capturing");
    if (h->d_work) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(h->d_work));
    }
    h->d_work = nullptr;
    h->work_bytes = 0;
    h->work_used = false;
    if (hipMalloc(&h->d_work, need) != hipSuccess)
        return fail(TSG_ERR_NOMEM, "hipMalloc of " + std::to_string(need) + " B work buffer failed");
    h->work_bytes = need;
    return TSG_OK;
}

// Grows the actquant scratch (grow-only, the rules of ensure_work): `rows`
// row scales of each kind, q8 bytes of int8 q.
int ensure_aq(tsg_tcsc *h, int rows, size_t q8, bool capturing)
{
    const size_t need = ((size_t)std::max(rows, 1) + 127) / 128 * 128;
    if (need <= h->aq_rows && q8 <= h->aq8_bytes) return TSG_OK;
    if (capturing)
        return fail(TSG_ERR_ARG, "M=" + std::to_string(rows) + " needs a larger activation-quantisation scratch "
                                 "during stream capture; call tcsc_hip_reserve(h, max_M) before capturing");
    if (h->d_aq || h->d_aq8) HIP_TRY(hipDeviceSynchronize());  // launches that may still read the old buffers
    if (need > h->aq_rows) {
        if (h->d_aq) HIP_TRY(hipFree(h->d_aq));
        h->d_aq = nullptr;
        h->aq_rows = 0;
        if (hipMalloc(&h->d_aq, 3 * need * sizeof(float)) != hipSuccess)
            return fail(TSG_ERR_NOMEM, "hipMalloc of the activation-quantisation scales failed");
        h->aq_rows = need;
    }
    if (q8 > h->aq8_bytes) {
        if (h->d_aq8) HIP_TRY(hipFree(h->d_aq8));
        h->d_aq8 = nullptr;
        h->aq8_bytes = 0;
        if (hipMalloc(&h->d_aq8, q8) != hipSuccess)
            return fail(TSG_ERR_NOMEM, "hipMalloc of " + std::to_string(q8) + " B of quantised activations failed");
        h->aq8_bytes = q8;
    }
    return TSG_OK;
}

// Folds finished event pairs into the totals.  `all` waits for every pending
// pair; otherwise only the oldest is waited for (ring full).
int harvest_timing(tsg_tcsc *h, bool all)
{
    int todo = all ? h->ring_count : (h->ring_count == tsg_tcsc::kRing ? 1 : 0);
    while (todo-- > 0) {
        const int i = (h->ring_head - h->ring_count + tsg_tcsc::kRing) % tsg_tcsc::kRing;
        HIP_TRY(hipEventSynchronize(h->ev1[i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]));
        h->total_ms += ms;
        h->launches += 1;
        h->ring_count--;
    }
    return TSG_OK;
}

int ensure_events(tsg_tcsc *h)
{
    if (h->ev0[0]) return TSG_OK;
    for (int i = 0; i < tsg_tcsc::kRing; i++) {
        HIP_TRY(hipEventCreate(&h->ev0[i]));
        HIP_TRY(hipEventCreate(&h->ev1[i]));
    }
    return TSG_OK;
}

// The timing ring's slot of a call on `s`: -1 when timing is off or the call
// is captured, else a slot whose ev0 is recorded here (after a harvest when
// the ring is full) and whose ev1 timing_end records after the kernel.
int timing_begin(tsg_tcsc *h, bool capturing, hipStream_t s, int &slot)
{
    slot = -1;
    if (!h->timing || capturing) return TSG_OK;
    const int rc = harvest_timing(h, false);
    if (rc) return rc;
    slot = h->ring_head;
    HIP_TRY(hipEventRecord(h->ev0[slot], s));
    return TSG_OK;
}

int timing_end(tsg_tcsc *h, int slot, hipStream_t s)
{
    if (slot < 0) return TSG_OK;
    HIP_TRY(hipEventRecord(h->ev1[slot], s));
    h->ring_head = (h->ring_head + 1) % tsg_tcsc::kRing;
    h->ring_count++;
    return TSG_OK;
}

// The handle's own non-blocking stream (host-pointer calls, probes without a
// call stream): created once at registration (create_impl), so threads never
// race to create it.
int handle_stream(tsg_tcsc *h, hipStream_t &s)
{
    if (!h->stream) return fail(TSG_ERR_HIP, "handle has no stream (registration did not complete)");
    s = h->stream;
    return TSG_OK;
}

// The handle's image of a shape (the planner's indices, tsg_plan.h)
tsg_tcsc::JitVariant &variant_of(tsg_tcsc *h, const JitShape &sh)
{
    if (sh.r64 && sh.half) return h->jv64h[tsg::width_index(sh.nw) - 1];
    return sh.r64 ? h->jv64[tsg::shape_index(sh.nw, sh.waves)] : h->jv[tsg::shape_index(sh)];
}

// Compiles and loads the image of one shape (registration, tcsc_hip_reserve,
// or the first call that picks it) and runs its probe on `s` -- the call's
// stream, or the handle's own non-blocking stream (nullptr) -- and
// synchronises that stream only.  Caller holds h->mu (or owns h exclusively).
int ensure_jit_variant(tsg_tcsc *h, const JitShape &sh, hipStream_t s)
{
    const int nw = sh.nw, waves = sh.waves;
    const bool far = sh.far, r64 = sh.r64, half = sh.half;
    if (tsg::shape_index(sh) < 0 || !(r64 ? tsg::jit64_width_ok(nw) : tsg::jit_width_ok(nw)) ||
        (r64 && (far || h->plan.B)) || (half && (!r64 || waves != 4 || nw >= tsg::kJitNW)))
        return fail(TSG_ERR_ARG, "unsupported jit stream width " + std::to_string(nw) + " x " + std::to_string(waves) +
                                 " waves" + (r64 ? (half ? " (64-row image, half ring)" : " (64-row image)") : ""));
    tsg_tcsc::JitVariant &v = variant_of(h, sh);
    if (v.mod.function) return TSG_OK;
    tsg::JitImage img;
    tsg::build_jit_code(h->csp.data(), h->csn.data(), h->rip.empty() ? nullptr : h->rip.data(),
                        h->rin.empty() ? nullptr : h->rin.data(), h->plan.K, h->plan.N, h->plan.B, img, nw, waves, far,
                        r64, half);
    // stream offsets (wcode) and the dispatcher's region literal are 32-bit
    if ((uint64_t)img.code.size() * 4 >= (1ull << 32) - (1ull << 20))
        return fail(TSG_ERR_RANGE, "jit image of " + std::to_string((uint64_t)img.code.size() * 4) +
                                       " B exceeds the 32-bit stream offsets; shard W's columns");
#ifdef TSG_DIAG
    if (!h->plan.B)
        if (const char *d = tsg::knob_value("TSG_JIT_DIAG")) {  // diagnostic code sharing (results WRONG)
            const size_t S = (size_t)waves;  // streams per column tile
            if (std::strstr(d, "simdpair"))  // waves w and w + S/2 (one SIMD) share w's stream
                for (size_t k = 0; k < img.wcode.size(); k++)
                    if (k % S >= S / 2) img.wcode[k] = img.wcode[k - S / 2];
            if (std::strstr(d, "samecode"))  // every column tile runs tile 0's streams
                for (size_t k = S; k < img.wcode.size(); k++) img.wcode[k] = img.wcode[k % S];
            if (std::strstr(d, "samewave"))  // every wave of a tile runs its wave 0's stream
                for (size_t k = 0; k < img.wcode.size(); k++) img.wcode[k] = img.wcode[k - k % S];
            if (std::strstr(d, "pairwave"))  // waves 2i and 2i+1 share a stream
                for (size_t k = 0; k < img.wcode.size(); k++) img.wcode[k] = img.wcode[k & ~(size_t)1];
        }
#endif
    DeviceGuard g(h->device);
    // the 64-row image's 4-wave streams: run by 8-wave workgroups of
    // half-masked wave pairs (TSG_JIT_PAIR=1, read at load: A/B)
    const char *pv = tsg::knob_value("TSG_JIT_PAIR");
    const bool pair = r64 && waves == 4 && !half && pv && pv[0] == '1';
    const std::string err = v.mod.load(img.code, nw, waves, r64, half, pair);
    if (!err.empty()) return fail(TSG_ERR_HIP, "jit kernel (width " + std::to_string(nw) + "): " + err);
    // from here a failed attempt unloads the module and frees the stream
    // table: the variant stays unbuilt, a retry starts clean
    auto drop = [&](int rc) {
        if (v.d_wcode) (void)hipFree(v.d_wcode);
        v.d_wcode = nullptr;
        v.mod.unload();
        return rc;
    };
    const size_t wb = img.wcode.size() * sizeof(uint32_t);
    if (hipMalloc(&v.d_wcode, std::max<size_t>(wb, 4)) != hipSuccess) {
        v.d_wcode = nullptr;
        return drop(fail(TSG_ERR_NOMEM, "hipMalloc of the jit stream table failed"));
    }
    if (hipMemcpy(v.d_wcode, img.wcode.data(), wb, hipMemcpyHostToDevice) != hipSuccess)
        return drop(fail(TSG_ERR_HIP, "upload of the jit stream table failed"));
    // probe launch: the dispatcher checks that its patched literal reaches the
    // generated region (magic header) and reports it; nothing else runs.  Done
    // here, at registration / reserve, so calls never read the status back
    // (they stay asynchronous and graph-capturable).
    if (!h->d_status && hipMalloc(&h->d_status, 16) != hipSuccess)
        return drop(fail(TSG_ERR_NOMEM, "hipMalloc of the jit status word failed"));
    uint32_t st[2] = {0xffffffffu, 0u};
    if (!s) {
        const int rs = handle_stream(h, s);
        if (rs) return drop(rs);
    }
    bool ok = hipMemsetAsync(h->d_status, 0, 16, s) == hipSuccess && tsg::launch_jit_probe(v.mod, h->d_status, s) == 0 &&
              hipMemcpyAsync(st, h->d_status, sizeof st, hipMemcpyDeviceToHost, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;
    if (!ok || st[0] != 0 || st[1] != tsg::kJitMagic0)
        return drop(fail(TSG_ERR_HIP, "jit kernel (width " + std::to_string(nw) + "): probe launch did not find the "
                                      "generated code region (status " + std::to_string(st[0]) + ")"));
    v.nw = nw;
    v.waves = waves;
    v.pair = pair;
    v.Npad = img.Npad;
    v.piece_rows = img.piece_rows;
    v.nch = img.nch;
    v.chunk = img.chunk;
    v.code_bytes = (int64_t)img.code.size() * 4;
    v.wcode_words = (int64_t)img.wcode.size();
    return TSG_OK;
}

// Ensures the image a weight-compiled plan picked.  An image the loader
// refuses (or whose probe fails) when nothing pinned it: this and later calls
// that pick it run the 128-row 64 x 8 image -- same result bit for bit,
// another speed -- so warn, mark the shape bad, plan again (the plan is now
// that image's) and load it.
int ensure_call_image(tsg_tcsc *h, int M, CallPlan &p, hipStream_t s)
{
    const int rc = ensure_jit_variant(h, p.shape, s);
    if (rc != TSG_ERR_HIP || !tsg::may_fall_back(h->plan, p.shape)) return rc;
    std::fprintf(stderr, "[ternary_spgemm] warning: %s; running the 128-row 64 x 8 image instead\n",
                 g_tsg_host_err.c_str());
    h->plan.bad_variants |= 1u << tsg::variant_bit(p.shape);
    p = tsg::plan_call(h->plan, M);
    return ensure_jit_variant(h, p.shape, s);
}

// X^T copies of a small-M image (tsg_internal.h ell_copy_offset): two for the
// 8-row tile's 4-lane columns when TSG_ELL_COPIES=2 (A/B), else one
int ell_copies(int v)
{
    static const int env = [] {
        const char *c = tsg::knob_value("TSG_ELL_COPIES");
        const char *lg = tsg::knob_value("TSG_ELL_LG");
        return c && c[0] == '2' && (!lg || std::atoi(lg) == 4) ? 2 : 1;
    }();
    return v == tsg::kEllTile8 ? env : 1;
}

// The bank-window schedule of the 8-row tile's image (tsg_internal.h
// kEllSchedZeroRows): TSG_ELL_SCHED=0 / 1 (A/B)
bool ell_sched(int v)
{
    static const int env = [] {
        const char *c = tsg::knob_value("TSG_ELL_SCHED");
        const char *lg = tsg::knob_value("TSG_ELL_LG");
        return c && c[0] == '1' && (!lg || std::atoi(lg) == 4) ? 1 : 0;
    }();
    return v == tsg::kEllTile8 && env && ell_copies(v) == 1;
}

// Builds and uploads the ELL image of a variant.  Caller holds h->mu.
int ensure_ell(tsg_tcsc *h, int v)
{
    tsg_tcsc::EllVariant &e = h->ell[v];
    if (e.ready) return TSG_OK;
    tsg::build_ell_image(h->csp.data(), h->csn.data(), h->rip.empty() ? nullptr : h->rip.data(),
                         h->rin.empty() ? nullptr : h->rin.data(), h->plan.K, h->plan.N, tsg::kEllMaxC[v], tsg::kEllTileM[v], e.img,
                         ell_copies(v), ell_sched(v));
    DeviceGuard g(h->device);
    const size_t eb = e.img.ent.size() * 4, tb = std::max<size_t>(e.img.tab.size() * 4, 8);
    // allocate and upload into locals; the variant owns them only once both
    // uploads succeeded (a failed attempt leaves nothing behind, a retry
    // starts clean)
    uint32_t *d_ent = nullptr, *d_tab = nullptr;
    auto drop = [&](int code, const char *msg) {
        if (d_ent) (void)hipFree(d_ent);
        if (d_tab) (void)hipFree(d_tab);
        return fail(code, msg);
    };
    if (hipMalloc(&d_ent, eb) != hipSuccess || hipMalloc(&d_tab, tb) != hipSuccess)
        return drop(TSG_ERR_NOMEM, "hipMalloc of the small-M (ELL) image failed");
    if (hipMemcpy(d_ent, e.img.ent.data(), eb, hipMemcpyHostToDevice) != hipSuccess ||
        (!e.img.tab.empty() && hipMemcpy(d_tab, e.img.tab.data(), e.img.tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return drop(TSG_ERR_HIP, "upload of the small-M (ELL) image failed");
    e.d_ent = d_ent;
    e.d_tab = d_tab;
    e.bytes = (int64_t)(eb + tb);
    std::vector<uint32_t>().swap(e.img.ent);
    std::vector<uint32_t>().swap(e.img.tab);
    e.ready = true;
    return TSG_OK;
}

// One device-pointer call: the two blocks its launchers take (tsg_internal.h)
// and what only this file reads.  run_dev owns it.
struct Call {
    tsg::XIn in;    // X, xtype, M, K; g: the gamma of a normquant call (may be null)
    tsg::YOut out;  // b, alpha, rs, cs, ep, Y, ytype, ldY, M, N, prelu, stream
    bool capturing = false;
    // an actquant call (tsg_actquant.h): X is quantised per row on the way in
    // (stage_begin), drs_out is the caller's copy of deq (may be null)
    bool quant = false;
    float *drs_out = nullptr;
    // a normquant call (tsg_norm.h): an actquant call whose X goes through an
    // RMSNorm with gamma in.g and eps first
    bool norm = false;
    float eps = 0.0f;
    hipStream_t s() const { return (hipStream_t)out.stream; }
};

// Before a call stages its X^T: the work buffer holds it (ensure_work), and
// X^T of the previous call may still be read by its kernel on another
// stream: this call's staging waits for it (same stream: stream order)
int work_begin(tsg_tcsc *h, const CallPlan &p, const Call &c)
{
    const int M = c.in.M;
    // (a walk has no X^T: it comes here for the actquant scratch alone)
    int rc = p.is_ell() ? TSG_OK : ensure_work(h, M, p.tile_m, p.chunk, c.capturing);
    if (!rc && c.quant)
        rc = ensure_aq(h, M, p.is_ell() ? std::max<size_t>((size_t)M * h->plan.K, 16) : 0, c.capturing);
    if (rc) return rc;
    if (!c.capturing && h->work_used && h->work_stream != c.s()) HIP_TRY(hipStreamWaitEvent(c.s(), h->work_ev, 0));
    return TSG_OK;
}

// After the kernel that reads X^T is enqueued: the event the next call on
// another stream waits for
// (a captured call's reads happen at replay time and are not tracked:
// a replay must not overlap calls on other streams,
// include/ternary_spgemm.h; the record of the last uncaptured call
// stays, so the next uncaptured call still waits for it)
int work_end(tsg_tcsc *h, const Call &c)
{
    if (c.capturing) return TSG_OK;
    HIP_TRY(hipEventRecord(h->work_ev, c.s()));
    h->work_stream = c.s();
    h->work_used = true;
    return TSG_OK;
}

// work_begin, then for an actquant call the row pass: the call's blocks take
// the scratch (tsg_tcsc::d_aq: inv and, of a normquant call, rn for the pass
// that reads X, deq as the row scale of the kernel that stores Y) and the pass
// fills them (deq also to the caller), for a walk (q8) also the int8 q
int stage_begin(tsg_tcsc *h, const CallPlan &p, Call &c, bool q8)
{
    const int rc = work_begin(h, p, c);
    if (rc || !c.quant) return rc;
    float *const deq = h->d_aq + h->aq_rows;
    c.in.inv = h->d_aq;
    c.in.rn = c.norm ? h->d_aq + 2 * h->aq_rows : nullptr;
    c.out.rs = deq;
    if (tsg::launch_row_absmax(c.in, deq, c.drs_out, q8 ? h->d_aq8 : nullptr, c.eps, c.s()) != 0)
        return fail(TSG_ERR_HIP, std::string("row pass launch: ") + hipGetErrorString(hipGetLastError()));
    return TSG_OK;
}

// small M: the ELL walk reads X in place, whatever its element type (no X^T
// staging, no work buffer)
int run_ell(tsg_tcsc *h, const CallPlan &p, Call &c)
{
    if (!h->ell[p.ell].ready && c.capturing)
        return fail(TSG_ERR_ARG, "M=" + std::to_string(c.in.M) + " runs the small-M kernel, whose image is not "
                                 "built yet; call tcsc_hip_reserve before capturing");
    int rc = ensure_ell(h, p.ell);
    if (rc) return rc;
    // an actquant call: the row pass writes q as int8 into the scratch, and the
    // walk runs on it as an int8-X call scaled by the scratch's deq
    if (c.quant) {
        rc = stage_begin(h, p, c, true);
        if (rc) return rc;
        c.in.X = h->d_aq8, c.in.xtype = tsg::kXI8;
    }
    int slot;
    rc = timing_begin(h, c.capturing, c.s(), slot);
    if (rc) return rc;
    const tsg_tcsc::EllVariant &v = h->ell[p.ell];
    tsg::EllDev e;
    e.ent = v.d_ent, e.tab = v.d_tab, e.K = h->plan.K;
    e.C = v.img.C, e.nch = v.img.nch, e.xb = v.img.xb, e.zr = v.img.zr;
    const int lrc = p.kernel == Kernel::kEllPc ? tsg::launch_tcsc_ell_pc(p.ell, c.in.X, c.in.xtype, e, c.out)
                                               : tsg::launch_tcsc_ell(p.ell, c.in.X, c.in.xtype, e, c.out);
    if (lrc != 0)
        return fail(TSG_ERR_HIP, std::string("small-M kernel launch: ") + hipGetErrorString(hipGetLastError()));
    rc = timing_end(h, slot, c.s());
    return rc || !c.quant ? rc : work_end(h, c);
}

// the register-X walk: X^T pass, then the kernel
int run_rx(tsg_tcsc *h, const CallPlan &p, Call &c)
{
    const int K = h->plan.K;
    const XtDims d = dims_for(c.in.M, K, p.tile_m, p.chunk);
    int rc = stage_begin(h, p, c, false);
    if (rc) return rc;
    if (K == 0) {
        // no X at all: chain is +0; X^T stays zero
        HIP_TRY(hipMemsetAsync(h->d_work, 0, (size_t)d.Mp * d.Kp * sizeof(float), c.s()));
    } else if (tsg::launch_transpose(c.in, h->d_work, d.Mp, d.Kp, c.s()) != 0) {
        return fail(TSG_ERR_HIP, std::string("transpose launch: ") + hipGetErrorString(hipGetLastError()));
    }
    int slot;
    rc = timing_begin(h, c.capturing, c.s(), slot);
    if (rc) return rc;
    if (tsg::launch_tcsc_rx(h->d_work, d.Mp, h->d_seg, h->d_ent, h->rimg.Npad, h->rimg.nch, c.out) != 0)
        return fail(TSG_ERR_HIP, std::string("tcsc launch: ") + hipGetErrorString(hipGetLastError()));
    rc = timing_end(h, slot, c.s());
    return rc ? rc : work_end(h, c);
}

// a weight-compiled image `jv` (loaded): X^T pass unless the image reads X
// itself, then the dispatcher
int run_jit(tsg_tcsc *h, const CallPlan &p, const tsg_tcsc::JitVariant &jv, Call &c)
{
    const int M = c.in.M, N = h->plan.N, K = h->plan.K;
    const bool r64 = p.kernel == Kernel::kJit64;
    const XtDims d = dims_for(M, K, p.tile_m, p.chunk);
    tsg::JitLaunch g;  // of the call, the image and the plan
    g.Mp = d.Mp, g.status = h->d_status;
    g.wcode = jv.d_wcode, g.Npad = jv.Npad, g.nch = jv.nch, g.tile_cols = jv.nw * jv.waves;
    g.waves = jv.pair ? 2 * jv.waves : jv.waves;  // waves launched per workgroup
    g.gn = p.gn, g.gm = p.gm, g.tmask = p.tmask, g.tile_m = p.tile_m, g.xtouch = p.xtouch, g.tnear = p.tnear;
    // the stream steps through X^T chunks with a 32-bit stride, and the grid
    // (one workgroup per M tile x column tile) must stay under 2^32 threads
    // (waves: the pair factor included; the logical ids are 32-bit in the kernel)
    // (= Mp / tile_m x Npad / cols, what launch_tcsc_jit derives for the kernel)
    const int64_t wgs = tsg::jit_tiles(M, N, p.tile_m, g.tile_cols);
    if ((int64_t)d.Mp * p.chunk * 4 >= (1ll << 31) || wgs * g.waves * 64 >= (1ll << 32) || wgs >= (1ll << 31))
        return fail(TSG_ERR_ARG, "M=" + std::to_string(M) + " is too large for one jit launch; split the rows");
    // the looping launch (TSG_JIT_LOOP; tsg_plan.cpp loop_wgs): that many
    // workgroups, each running every loop-th logical id
    g.loop_wgs = jv.pair ? 0 : tsg::loop_wgs(p.shape, wgs);
#ifdef TSG_DIAG
    if (const char *dv = tsg::knob_value("TSG_JIT_DIAG")) {  // results WRONG (timing studies)
        if (std::strstr(dv, "nostore")) g.lflags |= tsg::kJitDiagNoStore;
        if (std::strstr(dv, "onetile")) {  // the first round alone
            g.lflags |= tsg::kJitDiagOneTile;
            g.loop_wgs = (int)std::min<int64_t>(wgs, std::max(h->cus / 8 * 8, 8));
        }
    }
#endif
    // the 64-row image stages straight from row-major X (no X^T pass, no work
    // buffer) when every row starts 16-B aligned and the offsets fit 32 bits
    // (the image's DMA reads fp32: an X of another type is always staged, by
    // the pass that widens it -- also at shapes where an fp32 X needs no work
    // buffer, which tcsc_hip_reserve sizes for the staged copy regardless)
    // (an actquant call is staged too: its staging pass quantises)
    const bool direct = !c.quant && c.in.xtype == tsg::kXF32 &&
                        tsg::x_direct(h->plan, p.shape, jv.piece_rows, ((uintptr_t)c.in.X & 15) == 0, M);
    if (r64 && jv.chunk != p.chunk)  // the image and this call's X^T dims must agree (TSG_JIT_QBLOCK read at both)
        return fail(TSG_ERR_ARG, "64-row image built for " + std::to_string(jv.chunk) + "-row chunks, call expects " +
                                     std::to_string(p.chunk) + " (TSG_JIT_QBLOCK changed after the image was built)");
    int rc;
    if (direct) {  // no staging kernel: the dispatcher's DMA reads X (fp32) itself
        g.xrow = K;
        // row layout: the last chunk starts at K - 188, lastadj bytes below its
        // slot (tsg_internal.h jit64_row_kbase)
        if (jv.piece_rows == 0)
            g.lastadj = 4 * ((jv.nch - 1) * tsg::kJit64RowChunk - tsg::jit64_row_kbase(K, jv.nch, jv.nch - 1));
    } else {
        rc = stage_begin(h, p, c, false);
        if (rc) return rc;
        if (K == 0) {
            // no X at all: chain is +0; X^T stays zero
            HIP_TRY(hipMemsetAsync(h->d_work, 0, (size_t)d.Mp * d.Kp * sizeof(float), c.s()));
        } else if ((r64 ? tsg::launch_transpose_quads(c.in, h->d_work, d.Mp, d.Kp, jv.piece_rows, p.chunk, c.s())
                        : tsg::launch_transpose_pairs(c.in, h->d_work, d.Mp, d.Kp, c.s())) != 0) {
            return fail(TSG_ERR_HIP, std::string("transpose launch: ") + hipGetErrorString(hipGetLastError()));
        }
    }
    int slot;
    rc = timing_begin(h, c.capturing, c.s(), slot);
    if (rc) return rc;
    int launched[2] = {0, 0};
    // (the work buffer as stage_begin left it: it may have grown)
    if (tsg::launch_tcsc_jit(jv.mod, direct ? c.in.X : h->d_work, g, c.out, launched) != 0)
        return fail(TSG_ERR_HIP, std::string("tcsc launch: ") + hipGetErrorString(hipGetLastError()));
    h->last_grid = launched[0];
    h->last_tiles = launched[1];
    rc = timing_end(h, slot, c.s());
    if (rc || direct) return rc;
    return work_end(h, c);
}

int check_shape(const tsg_tcsc *h, int N, int K)
{
    if (N == h->plan.N && K == h->plan.K) return TSG_OK;
    return fail(TSG_ERR_ARG, "shape mismatch: handle has K=" + std::to_string(h->plan.K) + " N=" +
                                 std::to_string(h->plan.N) + ", call has K=" + std::to_string(K) +
                                 " N=" + std::to_string(N));
}

// What every device-pointer call refuses before anything is enqueued, in the
// order that decides which of two faults a call reports
int check_call(const tsg_tcsc *h, const Call &c)
{
    const tsg::XIn &in = c.in;
    const tsg::YOut &o = c.out;
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (c.norm && !(std::isfinite(c.eps) && c.eps > 0.0f))
        return fail(TSG_ERR_ARG, "eps=" + std::to_string(c.eps) + ": the normquant calls need a finite eps > 0");
    if (c.quant && in.xtype == tsg::kXI8)
        return fail(TSG_ERR_ARG, "xtype=3 (int8): the actquant and normquant calls quantise an fp32, fp16 or bf16 X; an int8 X "
                                 "goes to tcsc_hip_gemm_dev_scaled with its own scale");
    if (!tsg::xtype_ok(in.xtype))
        return fail(TSG_ERR_ARG,
                    "xtype=" + std::to_string(in.xtype) + " is not a tsg_xtype (0 fp32, 1 fp16, 2 bf16, 3 int8)");
    if (!tsg::ytype_ok(o.ytype))
        return fail(TSG_ERR_ARG, "ytype=" + std::to_string(o.ytype) + " is not a tsg_ytype (0 fp32, 1 fp16, 2 bf16)");
    const int rc = check_shape(h, o.N, in.K);
    if (rc) return rc;
    if (o.M < 0) return fail(TSG_ERR_ARG, "M < 0");
    if (o.ldY < o.N)  // rows would overlap
        return fail(TSG_ERR_ARG, "ldY=" + std::to_string(o.ldY) + " is less than N=" + std::to_string(o.N));
    if (o.M == 0 || o.N == 0) return TSG_OK;  // an empty call reads no pointer
    if (!o.Y || !o.b || (in.K > 0 && !in.X) || (o.prelu && !o.alpha))
        return fail(TSG_ERR_ARG, "null device pointer");
    return TSG_OK;
}

int run_dev(tsg_tcsc *h, Call c)
{
    const int rc0 = check_call(h, c);
    if (rc0 || c.out.M == 0 || c.out.N == 0) return rc0;
    const int M = c.in.M;
    DeviceGuard g(h->device);
    // One call at a time per handle: the X^T work buffer, the jit images and
    // the timing ring are shared by every stream that uses the handle.
    std::lock_guard<std::mutex> lk(h->mu);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(c.s(), &cap));
    c.capturing = cap != hipStreamCaptureStatusNone;
    CallPlan p = tsg::plan_call(h->plan, M);
    if (p.is_ell()) return run_ell(h, p, c);
    if (!p.is_jit()) return run_rx(h, p, c);
    if (!variant_of(h, p.shape).mod.function) {
        if (c.capturing)
            return fail(TSG_ERR_ARG, "M=" + std::to_string(M) + " runs the width-" + std::to_string(p.shape.nw) +
                                         " image, which is not compiled yet; call tcsc_hip_reserve before capturing");
        const int rc = ensure_call_image(h, M, p, c.s());
        if (rc) return rc;
    }
    return run_jit(h, p, variant_of(h, p.shape), c);
}

// The fields every device-pointer call has, in the order of the C signatures
Call dev_call(const void *dX, int xtype, const float *db, void *dY, int ytype, int64_t ldY, int M, int N, int K,
              void *stream)
{
    Call c;
    c.in.X = dX, c.in.xtype = xtype, c.in.M = M, c.in.K = K;
    c.out.b = db, c.out.Y = dY, c.out.ytype = ytype, c.out.ldY = ldY, c.out.M = M, c.out.N = N;
    c.out.stream = stream;
    return c;
}

// ... and what a _prelu, an _actquant and a _normquant call add
Call with_prelu(Call c, const float *dalpha)
{
    c.out.alpha = dalpha, c.out.prelu = true;
    return c;
}
Call with_quant(Call c, float *drow_scale_out, const float *dcol_scale)
{
    c.quant = true, c.drs_out = drow_scale_out, c.out.cs = dcol_scale;
    return c;
}
Call with_norm(Call c, const float *dgamma, float eps)
{
    c.norm = true, c.in.g = dgamma, c.eps = eps;
    return c;
}

int host_pipe_ready(tsg_tcsc *h)
{
    if (h->s_in) return TSG_OK;
    HIP_TRY(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    for (int i = 0; i < tsg::kHostChunksMax; i++) {
        HIP_TRY(hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_c[i], hipEventDisableTiming));
    }
    HIP_TRY(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));  // last: marks the pipeline ready
    return TSG_OK;
}

// The comp_func call (main.cpp:214-216): host X, b, Y; synchronous.  Pipelined
// by M chunks over three streams: the calling thread copies X chunk i in
// (s_in) and enqueues its compute (the handle's stream, after chunk i's copy)
// while a helper thread copies the finished Y chunks out (s_out, after each
// chunk's compute), so the H2D of chunk i+1, the kernel of chunk i and the
// D2H of chunk i-1 overlap (PCIe is full duplex).  Rows are independent, so
// the chunked result is the unchunked one bit for bit.
int run_host_impl(tsg_tcsc *h, const float *X, const float *b, const float *alpha, float *Y, int M, int N, int K,
                  bool prelu);

// No exception crosses the extern "C" boundary: a std::bad_alloc or
// std::system_error (thread creation) inside the pipeline becomes a status.
int run_host(tsg_tcsc *h, const float *X, const float *b, const float *alpha, float *Y, int M, int N, int K,
             bool prelu)
{
    try {
        return run_host_impl(h, X, b, alpha, Y, M, N, K, prelu);
    } catch (const std::bad_alloc &) {
        return fail(TSG_ERR_NOMEM, "host-pointer call: out of host memory");
    } catch (const std::exception &e) {
        return fail(TSG_ERR_HIP, std::string("host-pointer call: ") + e.what());
    }
}

int run_host_impl(tsg_tcsc *h, const float *X, const float *b, const float *alpha, float *Y, int M, int N, int K,
                  bool prelu)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (const int rc = check_shape(h, N, K)) return rc;
    if (M < 0) return fail(TSG_ERR_ARG, "M < 0");
    if (M == 0 || N == 0) return TSG_OK;
    if (!Y || !b || (K > 0 && !X) || (prelu && !alpha)) return fail(TSG_ERR_ARG, "null host pointer");
    DeviceGuard g(h->device);
    // the staging buffers and the streams are the handle's: a second host
    // thread waits here until this call's Y is back (run_dev takes h->mu inside)
    std::lock_guard<std::mutex> lk(h->host_mu);
    const size_t xb = (size_t)M * K * sizeof(float), yb = (size_t)M * N * sizeof(float);
    if (xb > h->x_bytes) {
        if (h->d_x) HIP_TRY(hipFree(h->d_x));
        h->d_x = nullptr;
        h->x_bytes = 0;
        if (hipMalloc(&h->d_x, std::max<size_t>(xb, 4)) != hipSuccess) return fail(TSG_ERR_NOMEM, "hipMalloc X");
        h->x_bytes = xb;
    }
    if (yb > h->y_bytes) {
        if (h->d_y) HIP_TRY(hipFree(h->d_y));
        h->d_y = nullptr;
        h->y_bytes = 0;
        if (hipMalloc(&h->d_y, yb) != hipSuccess) return fail(TSG_ERR_NOMEM, "hipMalloc Y");
        h->y_bytes = yb;
    }
    hipStream_t s = nullptr;
    int rc = handle_stream(h, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_b, b, (size_t)N * sizeof(float), hipMemcpyHostToDevice, s));
    if (prelu) HIP_TRY(hipMemcpyAsync(h->d_alpha, alpha, (size_t)N * sizeof(float), hipMemcpyHostToDevice, s));
    auto run_rows = [&](size_t r0, size_t nr) {  // the device call of rows [r0, r0 + nr) of the staged X
        Call c = dev_call(h->d_x + r0 * K, tsg::kXF32, h->d_b, h->d_y + r0 * N, tsg::kYF32, N, (int)nr, N, K, s);
        c.out.alpha = h->d_alpha, c.out.prelu = prelu;
        return run_dev(h, c);
    };
    const int rows = tsg::host_chunk_rows(h->plan, h->host_chunks, M);
    if (rows >= M) {
        if (xb) HIP_TRY(hipMemcpyAsync(h->d_x, X, xb, hipMemcpyHostToDevice, s));
        rc = run_rows(0, (size_t)M);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(Y, h->d_y, yb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TSG_OK;
    }
    rc = host_pipe_ready(h);
    if (rc) return rc;
    const int nchunk = (M + rows - 1) / rows;
    // chunks enqueued by this thread (their ev_c recorded); -1 = stop (error)
    std::mutex m;
    std::condition_variable cv;
    int enq = 0;
    hipError_t out_err = hipSuccess;
    // joins the helper on every path out of this scope (an exception included)
    struct Joiner {
        std::thread &t;
        std::mutex &m;
        std::condition_variable &cv;
        int &enq;
        ~Joiner()
        {
            if (!t.joinable()) return;
            {
                std::lock_guard<std::mutex> gl(m);
                enq = -1;
            }
            cv.notify_all();
            t.join();
        }
    };
    std::thread out([&] {
        DeviceGuard tg(h->device);
        for (int i = 0; i < nchunk && out_err == hipSuccess; i++) {
            {
                std::unique_lock<std::mutex> ul(m);
                cv.wait(ul, [&] { return enq > i || enq < 0; });
                if (enq < 0) break;
            }
            const size_t r0 = (size_t)i * rows, nr = std::min<size_t>(rows, (size_t)M - r0);
            out_err = hipStreamWaitEvent(h->s_out, h->ev_c[i], 0);
            if (out_err == hipSuccess)
                out_err = hipMemcpyAsync(Y + r0 * N, h->d_y + r0 * N, nr * N * sizeof(float), hipMemcpyDeviceToHost,
                                         h->s_out);
        }
        const hipError_t e = hipStreamSynchronize(h->s_out);
        if (out_err == hipSuccess) out_err = e;
    });
    Joiner joiner{out, m, cv, enq};
    auto stop = [&](int code) {
        {
            std::lock_guard<std::mutex> gl(m);
            if (code) enq = -1;
        }
        cv.notify_all();
        out.join();
        // on an error, chunks already enqueued may still read d_x / write d_y:
        // drain them so the next call's copies cannot overtake them
        if (code) (void)hipStreamSynchronize(s);
        return code;
    };
    for (int i = 0; i < nchunk; i++) {
        const size_t r0 = (size_t)i * rows, nr = std::min<size_t>(rows, (size_t)M - r0);
        hipError_t e = hipSuccess;
        if (K > 0) e = hipMemcpyAsync(h->d_x + r0 * K, X + r0 * K, nr * K * sizeof(float), hipMemcpyHostToDevice, h->s_in);
        if (e == hipSuccess) e = hipEventRecord(h->ev_in[i], h->s_in);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, h->ev_in[i], 0);
        if (e != hipSuccess) return stop(fail(TSG_ERR_HIP, std::string("host pipeline (X chunk): ") + hipGetErrorString(e)));
        rc = run_rows(r0, nr);
        if (rc) return stop(rc);
        e = hipEventRecord(h->ev_c[i], s);
        if (e != hipSuccess) return stop(fail(TSG_ERR_HIP, std::string("host pipeline (event): ") + hipGetErrorString(e)));
        {
            std::lock_guard<std::mutex> gl(m);
            enq = i + 1;
        }
        cv.notify_all();
    }
    stop(0);
    if (out_err != hipSuccess) {
        // chunks still queued on the compute stream may read d_x / write d_y:
        // drain them before the next call's copies can overwrite d_x
        (void)hipStreamSynchronize(s);
        return fail(TSG_ERR_HIP, std::string("host pipeline (Y chunk): ") + hipGetErrorString(out_err));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return TSG_OK;
}

void free_handle(tsg_tcsc *h)
{
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->ring_count) (void)hipDeviceSynchronize();
    if (h->work_ev) (void)hipEventDestroy(h->work_ev);
    for (void *p : {(void *)h->d_seg, (void *)h->d_ent, (void *)h->d_work, (void *)h->d_x,
                    (void *)h->d_b, (void *)h->d_y, (void *)h->d_alpha, (void *)h->d_status, (void *)h->d_aq,
                    (void *)h->d_aq8})
        if (p) (void)hipFree(p);
    for (auto *vs : {&h->jv[0], &h->jv64[0], &h->jv64h[0]})
        for (size_t i = 0; i < (vs == &h->jv[0] ? std::size(h->jv) : vs == &h->jv64[0] ? std::size(h->jv64)
                                                                                      : std::size(h->jv64h)); i++) {
            if (vs[i].d_wcode) (void)hipFree(vs[i].d_wcode);
            vs[i].mod.unload();
        }
    for (auto &e : h->ell) {
        if (e.d_ent) (void)hipFree(e.d_ent);
        if (e.d_tab) (void)hipFree(e.d_tab);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    for (int i = 0; i < tsg::kHostChunksMax; i++) {
        if (h->ev_in[i]) (void)hipEventDestroy(h->ev_in[i]);
        if (h->ev_c[i]) (void)hipEventDestroy(h->ev_c[i]);
    }
    for (int i = 0; i < tsg_tcsc::kRing; i++) {
        if (h->ev0[i]) (void)hipEventDestroy(h->ev0[i]);
        if (h->ev1[i]) (void)hipEventDestroy(h->ev1[i]);
    }
    delete h;
}

}  // namespace

// ================================================================ C-ABI ==

extern "C" const char *tcsc_hip_last_error(void)
{
    return g_tsg_host_err.c_str();
}

extern "C" int tcsc_hip_device_count(int *count)
{
    if (!count) return fail(TSG_ERR_ARG, "null count");
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail(TSG_ERR_NODEV, "hipGetDeviceCount failed");
    *count = n;
    return TSG_OK;
}

namespace {

// Registration of TCSC (B = 0) or BlockedTCSC<B> arrays.
int create_impl(const int32_t *csp, const int32_t *csn, const int32_t *rip, const int32_t *rin, int K, int N,
                int B, int device, tsg_tcsc **out)
{
    if (!out) return fail(TSG_ERR_ARG, "null out");
    *out = nullptr;
    if (B < 0) return fail(TSG_ERR_ARG, "negative block size");
    // a malformed environment knob (or, in the product build, the wrong-result
    // diagnostics of TSG_JIT_DIAG) is refused before anything else
    const std::string ke = tsg::knob_check();
    if (!ke.empty()) return fail(TSG_ERR_ARG, ke);
    std::string e = tsg::validate_tcsc(csp, csn, rip, rin, K, N, B);
    if (!e.empty()) return fail(TSG_ERR_ARG, std::string(B ? "malformed BlockedTCSC: " : "malformed TCSC: ") + e);
    if (B && (tsg::kJitXRegs - tsg::kJitNW) / tsg::kJitSlotRegs < 2)
        return fail(TSG_ERR_ARG, "BlockedTCSC: this jit kernel geometry has no registers for the block sums");
    const int64_t slots = (B ? (int64_t)(K / B) : 1) * N;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TSG_ERR_NODEV, "no HIP device");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(TSG_ERR_ARG, "device index out of range");
    int rc = check_device(device);
    if (rc) return rc;

    tsg_tcsc *h = new tsg_tcsc();
    h->plan.K = K;
    h->plan.N = N;
    h->plan.B = B;
    h->device = device;
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        h->cus = 0;  // (only the diagnostic one-round launch reads it)
    }
    {
        DeviceGuard g0(device);
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            delete h;
            return fail(TSG_ERR_HIP, "hipStreamCreate of the handle's stream failed");
        }
    }
    h->nnz_pos = csp[slots];
    h->nnz_neg = csn[slots];
    h->plan.nnz = h->nnz_pos + h->nnz_neg;
    h->csp.assign(csp, csp + slots + 1);
    h->csn.assign(csn, csn + slots + 1);
    if (h->nnz_pos) h->rip.assign(rip, rip + h->nnz_pos);
    if (h->nnz_neg) h->rin.assign(rin, rin + h->nnz_neg);
    // kernel family (default: the weight-compiled kernel); TSG_KERNEL selects
    // the others for A/B and their own tests
    const char *kenv = tsg::knob_value("TSG_KERNEL");
    // The weight-compiled image costs ~8 B per nonzero plus ~15% schedule code;
    // stream offsets are 32-bit, so a W whose image would pass ~3 GiB (e.g.
    // K=16384, N=131072, s=4 on ONE GPU -- shard columns instead)
    // defaults to the rx kernel.  Asking for jit explicitly is then an error.
    // A stream step (DMA, barrier, waits) costs ~256 B on top; BlockedTCSC walks
    // every block's chunks twice per column half.
    const int64_t nchk = std::max(1, (K + tsg::kJitChunk - 1) / tsg::kJitChunk);
    const int64_t steps = B ? 4 * (int64_t)(K / B) * ((B + tsg::kJitChunk - 1) / tsg::kJitChunk + 1) : 2 * nchk;
    const int64_t streams = (int64_t)((N + tsg::kJitTileCols - 1) / tsg::kJitTileCols) * tsg::kJitStreams;
    const double jit_est =
        8.0 * 1.25 * ((double)h->nnz_pos + (double)h->nnz_neg) + 256.0 * (double)steps * (double)streams;
    const bool jit_fits = jit_est < 3.0 * (double)(1ull << 30);
    const std::string kname = kenv ? kenv : (jit_fits ? "jit" : "rx");
    if (kname != "jit" && kname != "rx") {
        free_handle(h);  // destroys the handle's stream too
        return fail(TSG_ERR_ARG, "TSG_KERNEL=" + kname + ": expected jit or rx");
    }
    if (B && kname != "jit") {
        free_handle(h);
        return fail(TSG_ERR_ARG, "BlockedTCSC runs on the jit kernel only (TSG_KERNEL=" + kname + ")");
    }
    if ((kname == "jit" || B) && !jit_fits) {
        free_handle(h);
        return fail(TSG_ERR_ARG, "TSG_KERNEL=jit: W has too many nonzeros for one weight-compiled image "
                                 "(> ~300M); shard columns across handles or use TSG_KERNEL=rx");
    }
    h->plan.jit = kname == "jit";
    if (h->plan.jit) {
        // TSG_JIT_NW=<64|32|16|8> pins the stream width (A/B); default: per call
        if (const char *wv = tsg::knob_value("TSG_JIT_NW")) {
            const int nw = std::atoi(wv);
            if (tsg::width_index(nw) < 0 || !tsg::jit_width_ok(nw) || (B && nw != tsg::kJitNW)) {
                free_handle(h);
                return fail(TSG_ERR_ARG, std::string("TSG_JIT_NW=") + wv + ": expected 64, 32, 16 or 8 (64 for BlockedTCSC)");
            }
            h->plan.jit_force = nw;
        }
        // Registration compiles, loads and probes the image most calls run --
        // the 64-row image's 128 x 8 (configs[2] and the sparse end, M >= 1024
        // at N = 16384) -- so a handle does not also carry the 128-row image
        // (8 B per nonzero) unless a call picks it or falls back to it.  If the
        // 64-row image cannot load here, the 128-row 64 x 8 one is tried (calls
        // that pick a 64-row image then warn and fall back, run_dev), then rx.
        h->plan.jit_nch = std::max(1, (K + tsg::kJitChunk - 1) / tsg::kJitChunk);
        int rc0 = !B && !h->plan.jit_force && !tsg::knob_value("TSG_JIT_ROWS64_MAXM")
                      ? ensure_jit_variant(h, {tsg::kJit64WideNW, tsg::kJitWaves, false, true}, nullptr)
                      : TSG_ERR_ARG;
        if (rc0) rc0 = ensure_jit_variant(h, {h->plan.jit_force ? h->plan.jit_force : tsg::kJitNW, tsg::kJitWaves}, nullptr);
        if (rc0) {
            // A generated image that the loader refuses (or whose probe launch
            // does not find its region) falls back to the rx kernel, unless jit
            // was asked for explicitly or the format needs it (BlockedTCSC).
            if ((rc0 != TSG_ERR_HIP && rc0 != TSG_ERR_RANGE) || kenv || B) {
                free_handle(h);
                return rc0;
            }
            std::fprintf(stderr, "[ternary_spgemm] warning: weight-compiled image unavailable (%s); "
                                 "falling back to the rx kernel\n", g_tsg_host_err.c_str());
            h->plan.jit = false;
        }
    }
    if (!h->plan.jit) tsg::build_rx_image(csp, csn, rip, rin, K, N, h->rimg);
    static const std::vector<uint32_t> kNoEntries(1, 0u);
    const std::vector<uint32_t> *segv = !h->plan.jit ? &h->rimg.wstart : &kNoEntries;
    const std::vector<uint32_t> *entv = !h->plan.jit ? &h->rimg.ent : &kNoEntries;

    DeviceGuard g(device);
    const size_t sb = segv->size() * sizeof(uint32_t), eb = entv->size() * sizeof(uint32_t);
    if (hipMalloc(&h->d_seg, sb) != hipSuccess || hipMalloc(&h->d_ent, eb) != hipSuccess ||
        hipMalloc(&h->d_b, std::max<size_t>((size_t)N * sizeof(float), 4)) != hipSuccess ||
        hipMalloc(&h->d_alpha, std::max<size_t>((size_t)N * sizeof(float), 4)) != hipSuccess ||
        (!h->d_status && hipMalloc(&h->d_status, 16) != hipSuccess)) {
        free_handle(h);
        return fail(TSG_ERR_NOMEM, "hipMalloc of the device image failed");
    }
    if (hipEventCreateWithFlags(&h->work_ev, hipEventDisableTiming) != hipSuccess) {
        free_handle(h);
        return fail(TSG_ERR_HIP, "hipEventCreate of the work-buffer event failed");
    }
    if (hipMemset(h->d_status, 0, 16) != hipSuccess ||
        hipMemcpy(h->d_seg, segv->data(), sb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_ent, entv->data(), eb, hipMemcpyHostToDevice) != hipSuccess) {
        free_handle(h);
        return fail(TSG_ERR_HIP, "upload of the device image failed");
    }
    *out = h;
    return TSG_OK;
}

}  // namespace

extern "C" int tcsc_hip_create(const int32_t *csp, const int32_t *csn, const int32_t *rip,
                               const int32_t *rin, int K, int N, int device, tsg_tcsc **out)
{
    return create_impl(csp, csn, rip, rin, K, N, 0, device, out);
}

extern "C" int tcsc_hip_create_blocked(const int32_t *csp, const int32_t *csn, const int32_t *rip,
                                       const int32_t *rin, int K, int N, int B, int device, tsg_tcsc **out)
{
    if (B <= 0) {
        if (out) *out = nullptr;
        return fail(TSG_ERR_ARG, "block size must be positive");
    }
    return create_impl(csp, csn, rip, rin, K, N, B, device, out);
}

extern "C" int tcsc_hip_create_dense(const int32_t *W, int K, int N, int device, tsg_tcsc **out)
{
    if (!out) return fail(TSG_ERR_ARG, "null out");
    *out = nullptr;
    if (!W || K < 0 || N < 0) return fail(TSG_ERR_ARG, "bad dense matrix");
    // TCSC ctor (TCSC.h:13-41): column by column, +1 / -1 rows ascending
    std::vector<int32_t> csp, csn, rip, rin;
    csp.reserve((size_t)N + 1);
    csn.reserve((size_t)N + 1);
    for (int n = 0; n < N; n++) {
        csp.push_back((int32_t)rip.size());
        csn.push_back((int32_t)rin.size());
        for (int k = 0; k < K; k++) {
            const int32_t v = W[(size_t)k * N + n];
            if (v == 1) rip.push_back(k);
            else if (v == -1) rin.push_back(k);
        }
    }
    csp.push_back((int32_t)rip.size());
    csn.push_back((int32_t)rin.size());
    return tcsc_hip_create(csp.data(), csn.data(), rip.data(), rin.data(), K, N, device, out);
}

extern "C" int tcsc_hip_encode_dense_dev(const int32_t *dW, int K, int N, int32_t *d_csp, int32_t *d_csn,
                                         int32_t *d_rip, int64_t rip_cap, int32_t *d_rin, int64_t rin_cap,
                                         int64_t *nnz_pos, int64_t *nnz_neg, void *stream)
{
    if (K < 0 || N < 0 || !d_csp || !d_csn || !nnz_pos || !nnz_neg || (K > 0 && N > 0 && !dW))
        return fail(TSG_ERR_ARG, "tcsc_hip_encode_dense_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    size_t tmp_bytes = 0;
    if (tsg::encode_count(dW, K, N, d_csp, d_csn, nullptr, &tmp_bytes, s) != 0)
        return fail(TSG_ERR_HIP, "tcsc_hip_encode_dense_dev: scan workspace query failed");
    void *tmp = nullptr;
    HIP_TRY(hipMallocAsync(&tmp, std::max<size_t>(tmp_bytes, 4), s));
    const int rc = tsg::encode_count(dW, K, N, d_csp, d_csn, tmp, &tmp_bytes, s);
    HIP_TRY(hipFreeAsync(tmp, s));
    if (rc != 0) return fail(TSG_ERR_HIP, std::string("tcsc_hip_encode_dense_dev: count/scan: ") +
                                              hipGetErrorString(hipGetLastError()));
    int32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], d_csp + N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&tot[1], d_csn + N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *nnz_pos = tot[0];
    *nnz_neg = tot[1];
    if (!d_rip || !d_rin) return TSG_OK;
    if (rip_cap < tot[0] || rin_cap < tot[1])
        return fail(TSG_ERR_ARG, "tcsc_hip_encode_dense_dev: row index arrays too small");
    if (tsg::encode_fill(dW, K, N, d_csp, d_csn, d_rip, d_rin, s) != 0)
        return fail(TSG_ERR_HIP, std::string("tcsc_hip_encode_dense_dev: fill: ") + hipGetErrorString(hipGetLastError()));
    return TSG_OK;
}

extern "C" int tcsc_hip_create_csc_packed(const int32_t *col_ptr, const int32_t *row_idx,
                                          const uint8_t *packed, int K, int N, int device,
                                          tsg_tcsc **out)
{
    if (!out) return fail(TSG_ERR_ARG, "null out");
    *out = nullptr;
    int64_t p = 0, q = 0;
    int rc = tsg_csc_packed_to_tcsc(col_ptr, row_idx, packed, N, nullptr, nullptr, nullptr,
                                    nullptr, &p, &q);
    if (rc) return rc;
    std::vector<int32_t> csp((size_t)N + 1), csn((size_t)N + 1), rip((size_t)std::max<int64_t>(p, 1)),
        rin((size_t)std::max<int64_t>(q, 1));
    rc = tsg_csc_packed_to_tcsc(col_ptr, row_idx, packed, N, csp.data(), csn.data(), rip.data(),
                                rin.data(), &p, &q);
    if (rc) return rc;
    return tcsc_hip_create(csp.data(), csn.data(), rip.data(), rin.data(), K, N, device, out);
}

extern "C" void tcsc_hip_destroy(tsg_tcsc *h) { free_handle(h); }

// Prepares every call with M <= max_M: the work buffer for max_M rows and the
// image of every shape such a call picks (tsg_plan.cpp pick_jit_shape depends
// on M only through the number of 128-row M tiles).  After it, calls with M <=
// max_M allocate and compile nothing, so they can be captured in a graph.
// The work buffer is sized for the staged copy of every image whether or not
// an fp32 call would read X directly: a call with a narrower X (run_jit)
// always stages.
extern "C" int tcsc_hip_reserve(tsg_tcsc *h, int max_M)
{
    if (!h || max_M < 0) return fail(TSG_ERR_ARG, "bad reserve arguments");
    DeviceGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->mu);
    // the actquant scratch: the row scales of max_M rows, and the int8 q of the
    // largest M <= max_M that runs a small-M walk
    int walk_m = 0;
    for (int m = std::max(max_M, 1); m >= 1 && !walk_m; m--)
        if (tsg::plan_call(h->plan, m).is_ell()) walk_m = m;
    int rc = ensure_aq(h, max_M, walk_m ? std::max<size_t>((size_t)walk_m * h->plan.K, 16) : 0, false);
    if (rc) return rc;
    if (!h->plan.jit) return ensure_work(h, max_M, tsg::kRxTileM, tsg::kRxChunk, false);
    rc = ensure_work(h, max_M, tsg::kJitTileM, tsg::kJitChunk, false);
    // the 64-row image's k-quad X^T (same bytes or fewer)
    if (!rc) rc = ensure_work(h, max_M, tsg::kJit64TileM, tsg::jit64_chunk(false), false);
    if (rc) return rc;
    // the image choice and its shape depend on M only through the 64- / 128-row
    // M tiles (and the small-M rule): the first and last M of every 64-row
    // range cover every image a call with M <= max_M picks
    const int ranges = (std::max(max_M, 1) + tsg::kJit64TileM - 1) / tsg::kJit64TileM;
    for (int r = 1; r <= ranges; r++) {
        for (const int m : {(r - 1) * tsg::kJit64TileM + 1, std::min(std::max(max_M, 1), r * tsg::kJit64TileM)}) {
            CallPlan p = tsg::plan_call(h->plan, m);
            if (!p.is_jit()) continue;  // the small-M kernel (its images below)
            rc = ensure_call_image(h, m, p, nullptr);
            if (rc) return rc;
        }
    }
    // the small-M images calls with M <= max_M run: the choice only changes
    // at M = 1..4 (1-row tiles by M * N), past an M tile or past kEllMidM, so
    // trying those covers them all
    for (int i = -4; i <= tsg::kEllVariants; i++) {
        const int m = i < 0 ? -i : i == tsg::kEllVariants ? tsg::kEllMidM + 1 : tsg::kEllTileM[i] + 1;
        const int v = m <= std::max(max_M, 1) ? tsg::plan_call(h->plan, m).ell : -1;
        if (v >= 0) {
            rc = ensure_ell(h, v);
            if (rc) return rc;
        }
    }
    return TSG_OK;
}

extern "C" int tcsc_hip_set_jit_width(tsg_tcsc *h, int width)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (!h->plan.jit) return fail(TSG_ERR_ARG, "tcsc_hip_set_jit_width: not a jit handle");
    if (width != 0 && (!tsg::jit64_width_ok(width) || (h->plan.B && width != tsg::kJitNW)))
        return fail(TSG_ERR_ARG, "tcsc_hip_set_jit_width: expected 0 (auto), 128 (64-row image), 64, 32, 16 or 8 "
                                 "(64 for BlockedTCSC)");
    std::lock_guard<std::mutex> lk(h->mu);
    h->plan.jit_force = width;
    return TSG_OK;
}

extern "C" int tcsc_hip_jit_width(const tsg_tcsc *h, int M)
{
    if (!h || !h->plan.jit) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return tsg::plan_call(h->plan, M).shape.nw;
}

extern "C" int tcsc_hip_jit_waves(const tsg_tcsc *h, int M)
{
    if (!h || !h->plan.jit) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return tsg::plan_call(h->plan, M).shape.waves;
}

extern "C" int tcsc_hip_set_tile_rows(tsg_tcsc *h, int rows)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (rows != 0 && rows != 64 && rows != 128) return fail(TSG_ERR_ARG, "tcsc_hip_set_tile_rows: expected 0 (auto), 64 or 128");
    if (rows == 64 && (!h->plan.jit || h->plan.B))
        return fail(TSG_ERR_ARG, "tcsc_hip_set_tile_rows: the 64-row image computes plain TCSC on the jit kernel only");
    std::lock_guard<std::mutex> lk(h->mu);
    h->plan.tile_rows = rows;
    return TSG_OK;
}

extern "C" int tcsc_hip_call_launches(const tsg_tcsc *h, const float *dX, int M)
{
    if (!h || M <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const CallPlan p = tsg::plan_call(h->plan, M);
    if (p.is_ell()) return 1;
    if (p.kernel != Kernel::kJit64) return 2;
    // the image's layout as run_jit sees it (-1: not built yet)
    const tsg_tcsc::JitVariant &v = variant_of(const_cast<tsg_tcsc *>(h), p.shape);
    return tsg::x_direct(h->plan, p.shape, v.mod.function ? v.piece_rows : -1, ((uintptr_t)dX & 15) == 0, M) ? 1 : 2;
}

extern "C" int tcsc_hip_call_tile_rows(const tsg_tcsc *h, int M)
{
    if (!h || M <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const CallPlan p = tsg::plan_call(h->plan, M);
    return p.is_jit() ? p.tile_m : 0;
}

// Opt-in page-locking of a caller's host buffer (X or Y of repeated
// host-pointer calls): the copies of the pipeline then DMA straight from / to
// it instead of the runtime's pin-on-the-fly staging.  The caller keeps the
// buffer alive until tcsc_hip_host_unregister.
extern "C" int tcsc_hip_host_register(void *p, size_t bytes)
{
    if (!p || bytes == 0) return fail(TSG_ERR_ARG, "tcsc_hip_host_register: null pointer or zero size");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return TSG_OK;
}

extern "C" int tcsc_hip_host_unregister(void *p)
{
    if (!p) return fail(TSG_ERR_ARG, "tcsc_hip_host_unregister: null pointer");
    HIP_TRY(hipHostUnregister(p));
    return TSG_OK;
}

extern "C" int tcsc_hip_set_host_chunks(tsg_tcsc *h, int chunks)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (chunks < 0 || chunks > tsg::kHostChunksMax)
        return fail(TSG_ERR_ARG, "tcsc_hip_set_host_chunks: expected 0 (auto) .. " +
                                     std::to_string(tsg::kHostChunksMax));
    std::lock_guard<std::mutex> lk(h->host_mu);
    h->host_chunks = chunks;
    return TSG_OK;
}

extern "C" int tcsc_hip_host_chunk_rows(tsg_tcsc *h, int M)
{
    if (!h || M <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->host_mu);
    return tsg::host_chunk_rows(h->plan, h->host_chunks, M);
}

extern "C" int tcsc_hip_set_far(tsg_tcsc *h, int mode)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (mode < 0 || mode > 2) return fail(TSG_ERR_ARG, "tcsc_hip_set_far: expected 0 (auto), 1 (never) or 2 (always)");
    std::lock_guard<std::mutex> lk(h->mu);
    h->plan.far_mode = mode;
    return TSG_OK;
}

extern "C" int tcsc_hip_call_far(const tsg_tcsc *h, int M)
{
    if (!h || M <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return tsg::plan_call(h->plan, M).shape.far ? 1 : 0;
}

extern "C" int tcsc_hip_set_small_m(tsg_tcsc *h, int mode)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    if (mode < 0 || mode > 3)
        return fail(TSG_ERR_ARG, "tcsc_hip_set_small_m: expected 0 (auto), 1 (never), 2 (always) or 3 (always, "
                                 "without the producer/consumer walk)");
    if (mode >= 2 && (!h->plan.jit || h->plan.B))
        return fail(TSG_ERR_ARG, "tcsc_hip_set_small_m: the small-M kernel computes plain TCSC (BaseTCSC) only");
    std::lock_guard<std::mutex> lk(h->mu);
    h->plan.small_m = mode;
    return TSG_OK;
}

// what the planner reads of an unpinned plain-TCSC handle with K, N and nnz nonzeros
static tsg::PlanInput plain_input(int K, int N, int64_t nnz)
{
    tsg::PlanInput in;
    in.K = K;
    in.N = N;
    in.nnz = nnz;
    in.jit_nch = std::max(1, (K + tsg::kJitChunk - 1) / tsg::kJitChunk);
    return in;
}

// The automatic per-call plan of a plain-TCSC handle with K, N and nnz
// nonzeros (host only, no GPU: the function run_dev uses on a handle).
// kernel: 0 weight-compiled (128-row image), 1 ELL walk, 2 ELL
// producer/consumer walk, 3 weight-compiled 64-row image.
extern "C" int tsg_call_plan(int K, int N, int64_t nnz, int M, int *kernel, int *width, int *waves, int *far,
                             int *gn, int *gm, int *tmask)
{
    if (K < 0 || N <= 0 || nnz < 0 || nnz > (int64_t)K * N || M <= 0 || !kernel || !width || !waves || !far ||
        !gn || !gm || !tmask) {
        g_tsg_host_err = "tsg_call_plan: bad arguments";
        return TSG_ERR_ARG;
    }
    const CallPlan p = tsg::plan_call(plain_input(K, N, nnz), M);
    *kernel = p.kernel == Kernel::kEll ? 1 : p.kernel == Kernel::kEllPc ? 2 : p.kernel == Kernel::kJit64 ? 3 : 0;
    *width = p.shape.nw;
    *waves = p.shape.waves;
    *far = p.shape.far ? 1 : 0;
    *gn = p.gn;
    *gm = p.gm;
    *tmask = p.tmask;
    return TSG_OK;
}

// The launch grid of an M-row weight-compiled call of such a handle, with
// tile_rows and width pinned as tcsc_hip_set_tile_rows / _set_jit_width pin
// them (0: automatic): the workgroups run_jit asks launch_tcsc_jit for (the
// same jit_tiles and loop_wgs, tsg_plan.cpp), and in *tiles the logical ids
// they run.  Host only; tcsc_hip_last_launch reports what a call launched.
extern "C" int tsg_call_grid(int K, int N, int64_t nnz, int M, int tile_rows, int width, int *tiles)
{
    if (K < 0 || N <= 0 || nnz < 0 || nnz > (int64_t)K * N || M <= 0 || !tiles ||
        (tile_rows != 0 && tile_rows != 64 && tile_rows != 128) ||
        (width != 0 && width != 8 && width != 16 && width != 32 && width != 64 && width != 128) ||
        (width == 128 && tile_rows == 128)) {
        g_tsg_host_err = "tsg_call_grid: bad arguments";
        return -TSG_ERR_ARG;
    }
    const std::string ke = tsg::knob_check();
    if (!ke.empty()) {
        g_tsg_host_err = "tsg_call_grid: " + ke;
        return -TSG_ERR_ARG;
    }
    tsg::PlanInput in = plain_input(K, N, nnz);
    in.tile_rows = tile_rows;
    in.jit_force = width;
    in.small_m = 1;
    const CallPlan p = tsg::plan_call(in, M);
    if (!p.is_jit()) {
        g_tsg_host_err = "tsg_call_grid: not a weight-compiled call";
        return -TSG_ERR_ARG;
    }
    const int64_t t = tsg::jit_tiles(M, N, p.tile_m, p.shape.nw * p.shape.waves);
    const int g = tsg::loop_wgs(p.shape, t);
    *tiles = (int)t;
    return g ? g : (int)t;
}

// Workgroups of the handle's last weight-compiled launch and, in *tiles, the
// logical ids it passed to the kernel: what launch_tcsc_jit handed to the
// runtime (0 before the first such launch).
extern "C" int tcsc_hip_last_launch(const tsg_tcsc *h, int *tiles)
{
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (tiles) *tiles = h->last_tiles;
    return h->last_grid;
}

// Whether an M-row call of a plain-TCSC handle with K, N and nnz nonzeros
// spreads the generated code's per-group touches (tsg_plan.cpp pick_xtouch;
// host only).
extern "C" int tsg_call_xtouch(int K, int N, int64_t nnz, int M)
{
    if (K < 0 || N <= 0 || nnz < 0 || nnz > (int64_t)K * N || M <= 0) {
        g_tsg_host_err = "tsg_call_xtouch: bad arguments";
        return TSG_ERR_ARG;
    }
    return tsg::plan_call(plain_input(K, N, nnz), M).xtouch;
}

extern "C" const char *tcsc_hip_call_kernel(const tsg_tcsc *h, int M)
{
    if (!h) return "";
    std::lock_guard<std::mutex> lk(h->mu);
    switch (tsg::plan_call(h->plan, M).kernel) {
    case Kernel::kEllPc: return "tsg_tcsc_ell_pc_kernel";
    case Kernel::kEll: return "tsg_tcsc_ell_kernel";
    case Kernel::kJit64: return "tsg_jit64_kernel";
    case Kernel::kJit128: return "tsg_jit_kernel";
    case Kernel::kRx: break;
    }
    return "tsg_tcsc_rx_kernel";
}

extern "C" int64_t tcsc_hip_call_image_bytes(tsg_tcsc *h, int M)
{
    if (!h || M <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const CallPlan p = tsg::plan_call(h->plan, M);
    if (p.is_ell()) return h->ell[p.ell].ready ? h->ell[p.ell].bytes : 0;
    if (!p.is_jit()) return (int64_t)(h->rimg.wstart.size() + h->rimg.ent.size()) * 4;
    const tsg_tcsc::JitVariant &v = variant_of(h, p.shape);
    return v.mod.function ? v.code_bytes + v.wcode_words * 4 : 0;
}

extern "C" int tcsc_hip_gemm(tsg_tcsc *h, const float *X, const float *b, float *Y, int M, int N, int K)
{
    return run_host(h, X, b, nullptr, Y, M, N, K, false);
}

extern "C" int tcsc_hip_gemm_prelu(tsg_tcsc *h, const float *X, const float *b, const float *alpha,
                                   float *Y, int M, int N, int K)
{
    return run_host(h, X, b, alpha, Y, M, N, K, true);
}

extern "C" int tcsc_hip_gemm_dev(tsg_tcsc *h, const float *dX, const float *db, float *dY, int M,
                                 int N, int K, void *stream)
{
    return run_dev(h, dev_call(dX, tsg::kXF32, db, dY, tsg::kYF32, N, M, N, K, stream));
}

extern "C" int tcsc_hip_gemm_prelu_dev(tsg_tcsc *h, const float *dX, const float *db,
                                       const float *dalpha, float *dY, int M, int N, int K,
                                       void *stream)
{
    return run_dev(h, with_prelu(dev_call(dX, tsg::kXF32, db, dY, tsg::kYF32, N, M, N, K, stream), dalpha));
}

extern "C" int tcsc_hip_gemm_dev_ld(tsg_tcsc *h, const float *dX, const float *db, float *dY, int64_t ldY,
                                    int M, int N, int K, void *stream)
{
    return run_dev(h, dev_call(dX, tsg::kXF32, db, dY, tsg::kYF32, ldY, M, N, K, stream));
}

extern "C" int tcsc_hip_gemm_prelu_dev_ld(tsg_tcsc *h, const float *dX, const float *db, const float *dalpha,
                                          float *dY, int64_t ldY, int M, int N, int K, void *stream)
{
    return run_dev(h, with_prelu(dev_call(dX, tsg::kXF32, db, dY, tsg::kYF32, ldY, M, N, K, stream), dalpha));
}

// X of another element type (tsg_xtype): the same calls, the type carried to
// the pass that reads X (XIn::xtype); TSG_X_F32 is tcsc_hip_gemm_dev_ld
extern "C" int tcsc_hip_gemm_dev_x(tsg_tcsc *h, const void *dX, int xtype, const float *db, float *dY, int64_t ldY,
                                   int M, int N, int K, void *stream)
{
    return run_dev(h, dev_call(dX, xtype, db, dY, tsg::kYF32, ldY, M, N, K, stream));
}

extern "C" int tcsc_hip_gemm_prelu_dev_x(tsg_tcsc *h, const void *dX, int xtype, const float *db,
                                         const float *dalpha, float *dY, int64_t ldY, int M, int N, int K,
                                         void *stream)
{
    return run_dev(h, with_prelu(dev_call(dX, xtype, db, dY, tsg::kYF32, ldY, M, N, K, stream), dalpha));
}

// Y of another element type (tsg_ytype): the same calls again, the type carried
// to the epilogue of the kernel that stores Y (YOut::ytype); TSG_Y_F32 is
// tcsc_hip_gemm_dev_x
extern "C" int tcsc_hip_gemm_dev_xy(tsg_tcsc *h, const void *dX, int xtype, const float *db, void *dY, int ytype,
                                    int64_t ldY, int M, int N, int K, void *stream)
{
    return run_dev(h, dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream));
}

extern "C" int tcsc_hip_gemm_prelu_dev_xy(tsg_tcsc *h, const void *dX, int xtype, const float *db,
                                          const float *dalpha, void *dY, int ytype, int64_t ldY, int M, int N, int K,
                                          void *stream)
{
    return run_dev(h, with_prelu(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), dalpha));
}

// The epilogue scales (tsg_scale.h): the _xy calls again with a per-row and a
// per-column scale between the chain and + b[n] (YOut::rs, YOut::cs); with
// both null they are the _xy calls
extern "C" int tcsc_hip_gemm_dev_scaled(tsg_tcsc *h, const void *dX, int xtype, const float *drow_scale,
                                        const float *dcol_scale, const float *db, void *dY, int ytype, int64_t ldY,
                                        int M, int N, int K, void *stream)
{
    Call c = dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream);
    c.out.rs = drow_scale, c.out.cs = dcol_scale;
    return run_dev(h, c);
}

extern "C" int tcsc_hip_gemm_prelu_dev_scaled(tsg_tcsc *h, const void *dX, int xtype, const float *drow_scale,
                                              const float *dcol_scale, const float *db, const float *dalpha, void *dY,
                                              int ytype, int64_t ldY, int M, int N, int K, void *stream)
{
    Call c = with_prelu(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), dalpha);
    c.out.rs = drow_scale, c.out.cs = dcol_scale;
    return run_dev(h, c);
}

// Fused per-row int8 activation quantisation (tsg_actquant.h): the _scaled
// calls on q = quantised X with drow_scale = deq, both made here -- the row
// pass finds deq, the staging pass quantises (Call::quant, Call::drs_out)
extern "C" int tcsc_hip_gemm_dev_actquant(tsg_tcsc *h, const void *dX, int xtype, float *drow_scale_out,
                                          const float *dcol_scale, const float *db, void *dY, int ytype, int64_t ldY,
                                          int M, int N, int K, void *stream)
{
    return run_dev(h, with_quant(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), drow_scale_out, dcol_scale));
}

extern "C" int tcsc_hip_gemm_prelu_dev_actquant(tsg_tcsc *h, const void *dX, int xtype, float *drow_scale_out,
                                                const float *dcol_scale, const float *db, const float *dalpha,
                                                void *dY, int ytype, int64_t ldY, int M, int N, int K, void *stream)
{
    const Call c = with_prelu(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), dalpha);
    return run_dev(h, with_quant(c, drow_scale_out, dcol_scale));
}

// Fused RMSNorm + activation quantisation (tsg_norm.h): the _actquant calls on
// xn = (X * rn[m]) * gamma[k], made by the same two passes -- the row pass finds
// rn first, the staging pass normalises what it loads before it quantises
// (Call::norm, XIn::g, Call::eps)
extern "C" int tcsc_hip_gemm_dev_normquant(tsg_tcsc *h, const void *dX, int xtype, const float *dgamma, float eps,
                                           float *drow_scale_out, const float *dcol_scale, const float *db, void *dY,
                                           int ytype, int64_t ldY, int M, int N, int K, void *stream)
{
    const Call c = with_quant(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), drow_scale_out, dcol_scale);
    return run_dev(h, with_norm(c, dgamma, eps));
}

extern "C" int tcsc_hip_gemm_prelu_dev_normquant(tsg_tcsc *h, const void *dX, int xtype, const float *dgamma, float eps,
                                                 float *drow_scale_out, const float *dcol_scale, const float *db,
                                                 const float *dalpha, void *dY, int ytype, int64_t ldY, int M, int N,
                                                 int K, void *stream)
{
    const Call c = with_prelu(dev_call(dX, xtype, db, dY, ytype, ldY, M, N, K, stream), dalpha);
    return run_dev(h, with_norm(with_quant(c, drow_scale_out, dcol_scale), dgamma, eps));
}

// The descriptor call (include/ternary_spgemm.h tsg_gemm_ex): every device call
// above as one struct that maps onto Call, plus the fused epilogue
// (tsg_epilogue.h).  The checks are host arithmetic on the descriptor alone, so
// that they can be tested without a device.
static_assert(sizeof(tsg_gemm_ex) == 144 && offsetof(tsg_gemm_ex, reserved) == 136, "the layout the header spells out");
static_assert(TSG_ACT_RELU == tsg::kEpiRelu && TSG_ACT_RELU2 == tsg::kEpiRelu2, "act values in Epi::bits");
extern "C" int tsg_gemm_ex_check(const tsg_gemm_ex *d, int M, int N, int K)
{
    (void)M;
    (void)K;
    if (!d) return fail(TSG_ERR_ARG, "d: null descriptor");
    if (d->struct_size != sizeof(tsg_gemm_ex))
        return fail(TSG_ERR_ARG, "struct_size=" + std::to_string(d->struct_size) + " is not sizeof(tsg_gemm_ex) = " +
                                     std::to_string(sizeof(tsg_gemm_ex)));
    if (d->reserved != 0) return fail(TSG_ERR_ARG, "reserved must be 0");
    if (d->in_mode < TSG_IN_PLAIN || d->in_mode > TSG_IN_NORMQUANT)
        return fail(TSG_ERR_ARG, "in_mode=" + std::to_string(d->in_mode) +
                                     " is not a tsg_in_mode (0 plain, 1 actquant, 2 normquant)");
    if (d->act < TSG_ACT_NONE || d->act > TSG_ACT_RELU2)
        return fail(TSG_ERR_ARG, "act=" + std::to_string(d->act) + " is not a tsg_act (0 none, 1 prelu, 2 relu, 3 relu2)");
    if (!tsg::xtype_ok(d->xtype))
        return fail(TSG_ERR_ARG,
                    "xtype=" + std::to_string(d->xtype) + " is not a tsg_xtype (0 fp32, 1 fp16, 2 bf16, 3 int8)");
    if (!tsg::ytype_ok(d->ytype))
        return fail(TSG_ERR_ARG, "ytype=" + std::to_string(d->ytype) + " is not a tsg_ytype (0 fp32, 1 fp16, 2 bf16)");
    if (!tsg::ytype_ok(d->multype))
        return fail(TSG_ERR_ARG, "multype=" + std::to_string(d->multype) + " is not a tsg_ytype (0 fp32, 1 fp16, 2 bf16)");
    if (!tsg::ytype_ok(d->addtype))
        return fail(TSG_ERR_ARG, "addtype=" + std::to_string(d->addtype) + " is not a tsg_ytype (0 fp32, 1 fp16, 2 bf16)");
    if (d->ldY < N) return fail(TSG_ERR_ARG, "ldY=" + std::to_string(d->ldY) + " is less than N=" + std::to_string(N));
    if (d->dmul && d->ldmul < N)
        return fail(TSG_ERR_ARG, "ldmul=" + std::to_string(d->ldmul) + " is less than N=" + std::to_string(N));
    if (d->dadd && d->ldadd < N)
        return fail(TSG_ERR_ARG, "ldadd=" + std::to_string(d->ldadd) + " is less than N=" + std::to_string(N));
    if (d->act == TSG_ACT_PRELU && !d->dalpha) return fail(TSG_ERR_ARG, "dalpha is NULL and act is TSG_ACT_PRELU");
    const bool quant = d->in_mode != TSG_IN_PLAIN, norm = d->in_mode == TSG_IN_NORMQUANT;
    if (quant && d->xtype == TSG_X_I8)
        return fail(TSG_ERR_ARG, "xtype=3 (int8): the quantising in_modes take an fp32, fp16 or bf16 X; an int8 X goes "
                                 "to TSG_IN_PLAIN with its own drow_scale");
    if (norm && !(std::isfinite(d->eps) && d->eps > 0.0f))
        return fail(TSG_ERR_ARG, "eps=" + std::to_string(d->eps) + ": TSG_IN_NORMQUANT needs a finite eps > 0");
    if (!norm && d->dgamma) return fail(TSG_ERR_ARG, "dgamma belongs to TSG_IN_NORMQUANT and must be NULL in this in_mode");
    if (quant && d->drow_scale)
        return fail(TSG_ERR_ARG, "drow_scale belongs to TSG_IN_PLAIN and must be NULL in the quantising in_modes");
    if (!quant && d->drow_scale_out)
        return fail(TSG_ERR_ARG, "drow_scale_out belongs to the quantising in_modes and must be NULL in TSG_IN_PLAIN");
    return TSG_OK;
}

extern "C" int tcsc_hip_gemm_dev_ex(tsg_tcsc *h, const tsg_gemm_ex *d, int M, int N, int K, void *stream)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    const int rc = tsg_gemm_ex_check(d, M, N, K);
    if (rc) return rc;
    // the epilogue as the kernels take it; an operand that is exactly Y (the
    // in-place form) is marked, so that the kernel loads it through Y itself
    tsg::Epi ep;
    if (d->act >= TSG_ACT_RELU) ep.bits |= d->act;  // kEpiRelu, kEpiRelu2
    if (d->dmul) {
        ep.mul = d->dmul;
        ep.ldmul = d->ldmul;
        ep.bits |= d->multype << tsg::kEpiMulShift;
        if (d->dmul == d->dY && d->multype == d->ytype && d->ldmul == d->ldY) ep.bits |= tsg::kEpiMulIsY;
    }
    if (d->dadd) {
        ep.add = d->dadd;
        ep.ldadd = d->ldadd;
        ep.bits |= d->addtype << tsg::kEpiAddShift;
        if (d->dadd == d->dY && d->addtype == d->ytype && d->ldadd == d->ldY) ep.bits |= tsg::kEpiAddIsY;
    }
    Call c = dev_call(d->dX, d->xtype, d->db, d->dY, d->ytype, d->ldY, M, N, K, stream);
    if (d->act == TSG_ACT_PRELU) c = with_prelu(c, d->dalpha);
    c.out.rs = d->drow_scale, c.out.cs = d->dcol_scale, c.out.ep = ep;
    c.quant = d->in_mode != TSG_IN_PLAIN, c.drs_out = d->drow_scale_out;
    c.norm = d->in_mode == TSG_IN_NORMQUANT, c.in.g = d->dgamma, c.eps = d->eps;
    return run_dev(h, c);
}

extern "C" int tcsc_hip_info(const tsg_tcsc *h, tsg_info *o)
{
    if (!h || !o) return fail(TSG_ERR_ARG, "null argument");
    std::memset(o, 0, sizeof(*o));
    o->K = h->plan.K;
    o->N = h->plan.N;
    o->device = h->device;
    o->abi_version = TSG_ABI_VERSION;
    o->nnz_pos = h->nnz_pos;
    o->nnz_neg = h->nnz_neg;
    // TCSC / BlockedTCSC getDataStructureSize (TCSC.h:43-49, BlockedTCSC.h:43-47)
    o->tcsc_bytes = 4 * (2 * (int64_t)h->csp.size() + h->nnz_pos + h->nnz_neg);
    const bool jit = h->plan.jit;
    int64_t jit_bytes = 0;
    for (const auto &v : h->jv) jit_bytes += v.code_bytes + v.wcode_words * 4;
    for (const auto &v : h->jv64) jit_bytes += v.code_bytes + v.wcode_words * 4;
    for (const auto &v : h->jv64h) jit_bytes += v.code_bytes + v.wcode_words * 4;
    for (const auto &e : h->ell) jit_bytes += e.bytes;
    o->image_bytes = jit ? jit_bytes : (int64_t)(h->rimg.wstart.size() + h->rimg.ent.size()) * 4;
    o->work_bytes = (int64_t)h->work_bytes;
    // the image registration loaded: the 64-row image's 128 x 8 when it could
    // (create_impl), else the 128-row 64 x 8 one (or rx)
    const tsg_tcsc::JitVariant &r64 = h->jv64[tsg::shape_index(tsg::kJit64WideNW, tsg::kJitWaves, false)];
    const bool reg64 = jit && r64.mod.function;
    o->chunk_rows = reg64 ? r64.chunk : jit ? tsg::kJitChunk : tsg::kRxChunk;
    o->tile_rows = reg64 ? tsg::kJit64TileM : jit ? tsg::kJitTileM : tsg::kRxTileM;
    o->tile_cols = reg64 ? tsg::kJit64WideNW * tsg::kJitWaves : jit ? tsg::kJitTileCols : tsg::kRxTileCols;
    return TSG_OK;
}

extern "C" const char *tcsc_hip_kernel_name(const tsg_tcsc *h)
{
    if (!h) return "";
    return h->plan.jit ? "tsg_jit_kernel" : "tsg_tcsc_rx_kernel";
}

extern "C" int tcsc_hip_to_dense(const tsg_tcsc *h, int32_t *W, int K, int N)
{
    if (!h || !W || K != h->plan.K || N != h->plan.N) return fail(TSG_ERR_ARG, "bad to_dense arguments");
    std::memset(W, 0, sizeof(int32_t) * (size_t)K * N);
    const size_t slots = h->csp.size() - 1;  // N, or (K/B)*N for BlockedTCSC (slot s: column s % N)
    for (size_t s = 0; s < slots; s++) {
        const size_t n = s % (size_t)N;
        for (int32_t i = h->csp[s]; i < h->csp[s + 1]; i++) W[(size_t)h->rip[i] * N + n] = 1;
        for (int32_t i = h->csn[s]; i < h->csn[s + 1]; i++) W[(size_t)h->rin[i] * N + n] = -1;
    }
    return TSG_OK;
}

extern "C" int tcsc_hip_set_timing(tsg_tcsc *h, int enable)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    int rc = enable ? ensure_events(h) : harvest_timing(h, true);
    if (rc) return rc;
    h->timing = enable != 0;
    return TSG_OK;
}

extern "C" int tcsc_hip_kernel_time(tsg_tcsc *h, double *total_ms, int64_t *launches, int reset)
{
    if (!h) return fail(TSG_ERR_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    int rc = harvest_timing(h, true);
    if (rc) return rc;
    if (total_ms) *total_ms = h->total_ms;
    if (launches) *launches = h->launches;
    if (reset) {
        h->total_ms = 0.0;
        h->launches = 0;
    }
    return TSG_OK;
}
