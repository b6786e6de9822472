// tsg_plan.h -- the per-call planner: which kernel, image, stream shape, tile
// map and touch settings a call with M rows takes.  Pure host arithmetic on a
// handle's K, N, B, nnz and pins (tsg_plan.cpp): no HIP, no handle, no heap,
// no lock (the caller holds the handle's).
#pragma once

#include <cstdint>

namespace tsg {

// A weight-compiled image: stream width x waves per workgroup, and which image
struct JitShape {
    int nw, waves;
    bool far = false;  // the far-X^T code image (tsg_jit.cpp build_jit_code)
    bool r64 = false;  // the 64-row image (tsg_internal.h)
    bool half = false; // its half ring (4-wave shapes; tsg_internal.h kJit64HalfChunk)
};

// A shape's index in a handle's tables of images (-1: no such shape) and its
// bit in PlanInput::bad_variants (tsg_plan.cpp)
int width_index(int nw);
int shape_index(int nw, int waves, bool far = false);
int shape_index(const JitShape &sh);
int variant_bit(const JitShape &sh);

// What the planner reads of a handle.  The handle keeps one (tsg_capi.cpp
// tsg_tcsc::plan) and its setters write the pins there.
struct PlanInput {
    int K = 0, N = 0;
    int B = 0;                  // BlockedTCSC<B> block size (0: plain TCSC)
    int64_t nnz = 0;            // +1 and -1 entries together
    bool jit = true;            // weight-compiled handle (false: the rx kernel)
    int tile_rows = 0;          // tcsc_hip_set_tile_rows: 0 auto, 128 or 64 (jit images)
    int jit_force = 0;          // tcsc_hip_set_jit_width / TSG_JIT_NW: 0 = auto
    int far_mode = 0;           // tcsc_hip_set_far: 0 auto, 1 never, 2 always (64 x 8 calls)
    int small_m = 0;            // tcsc_hip_set_small_m: 0 auto, 1 never, 2 always, 3 always w/o pc (plain TCSC only)
    // images that failed to load or probe at a call (bit variant_bit): calls
    // that pick them run the 128-row 64 x 8 image (loaded on that fallback)
    uint32_t bad_variants = 0;
    int jit_nch = 0;            // X^T chunks of the 128-row images (all widths)
};

enum class Kernel { kRx, kJit128, kJit64, kEll, kEllPc };

struct CallPlan {
    Kernel kernel = Kernel::kRx;
    int ell = -1;               // the walks: the small-M variant (tsg_internal.h kEllTileM)
    JitShape shape{0, 0};       // the weight-compiled images: the image the call runs
    int tile_m = 0, chunk = 0;  // X^T: rows per M tile and K rows per chunk (0: the walks read X in place)
    int gn = 0, gm = 0, tmask = 0;  // weight-compiled: tile map groups and code-touch mask (tsg_jit_map.h)
    int tnear = 0;              // weight-compiled: the code-touch window starts at the step's own position
    int xtouch = 0;             // the code-touch spreading rule's answer for this M (the weight-compiled launch reads it)
    bool is_ell() const { return kernel == Kernel::kEll || kernel == Kernel::kEllPc; }
    bool is_jit() const { return kernel == Kernel::kJit128 || kernel == Kernel::kJit64; }
};

CallPlan plan_call(const PlanInput &in, int M);

// Logical workgroup ids of a weight-compiled call: M tiles x column tiles
// (cols = stream width x streams per workgroup)
int64_t jit_tiles(int M, int N, int tile_m, int cols);

// The looping launch (tsg_jit_kernel.hip): the workgroups G a
// call on the image `sh` with `tiles` logical ids launches when each is to
// run several ids -- b, b + G, ... --; 0: one workgroup per id.  Only the
// 64-row image's 8-wave workgroups can loop, and only with more ids than G.
// G is TSG_JIT_LOOP (1..4096, read per call; a multiple of 8 keeps every id
// on its XCD, tsg_jit_map.h; tests loop tiny shapes with small values); unset
// or 0, no call loops.  A launch decision, not part of the CallPlan: the tile
// map, the touch mask and the image are those of the unlooped call.
int loop_wgs(const JitShape &sh, int64_t tiles);

// Whether a call on the image `sh` reads X directly (no X^T pass; 64-row
// image only): depends on the call's X (rows 16-B aligned) and on the built
// image's layout -- piece_rows, or -1 for an image not built yet (then the
// layout it would be built with).
bool x_direct(const PlanInput &in, const JitShape &sh, int piece_rows, bool x_aligned, int M);

// whether a call may run the 128-row 64 x 8 image when `sh` cannot be loaded
bool may_fall_back(const PlanInput &in, const JitShape &sh);

// The small-M variant with 8-row tiles, and the M up to which 8-row tiles
// are used (pick_ell_variant; the image builder and tcsc_hip_reserve's sweep
// read them too)
constexpr int kEllTile8 = 2;
constexpr int kEllMidM = 32;

// rows per chunk of the host-pointer pipeline (host_chunks: tcsc_hip_set_host_chunks, 0 = automatic)
constexpr int kHostChunksMax = 16;
int host_chunk_rows(const PlanInput &in, int host_chunks, int M);

}  // namespace tsg
