// mv_internal.hpp -- shared internals of libmaveric_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <initializer_list>

#include "maveric_hip.h"
#include "mv_carve.hpp"

// A grow-only device buffer of a context (mv::grow)
struct mv_buffer {
    void *p;
    size_t bytes;
};

// The batch the last all-pairs prepare recorded: the run entry points check their arguments
// against it.  desc1 == nullptr: nothing prepared.
struct mv_prepared {
    int batch, cap;
    const int *n1;
    const float *desc1;
    int screen;   // the context's screen at the prepare
    bool staged;  // frame 1 sits staged in ap_image (false: recorded only)
    void record(int batch_, int cap_, const int *n1_, const float *desc1_, int screen_, bool staged_) {
        batch = batch_, cap = cap_, n1 = n1_, desc1 = desc1_, screen = screen_, staged = staged_;
    }
    void invalidate() { desc1 = nullptr; }  // the image is overwritten or freed
    bool matches(int batch_, int cap_, const int *n1_, const float *desc1_) const {
        return desc1 && batch == batch_ && cap == cap_ && n1 == n1_ && desc1 == desc1_;
    }
};

struct mv_context {
    int device;
    hipStream_t own_stream;
    hipStream_t stream;  // where every *_dev launch goes
    mv_buffer scratch;   // device scratch, grown by mv::scratch() / mv_context_reserve()
    mv_buffer stage;     // small host<->device staging for the single-pair host entry points
    // all-pairs fp32 (mv_allpairs.hip): its own images (frame 1 as fp16 or int8, norms, range
    // flags) so that a prepare of the next batch on aux_stream never races the pose kernels on
    // `stream`; ap_image2 is the other image of run_prepare (swapped with ap_image per call)
    mv_buffer ap_image, ap_image2;
    hipStream_t aux_stream;  // created on first prepare, with ev_in and ev_prep
    hipEvent_t ev_in, ev_prep;
    mv_prepared prep;
    int ap_screen;  // mv_allpairs_screen of the fp32 all-pairs match (0 = int8, the default)
    // set_stream / use_own_stream away from a stream record this event on it and make own_stream
    // wait on it: own_stream then orders after all work issued on every stream the context left
    // (no stream handle is kept, so a caller may destroy a stream once the context moved off it)
    hipEvent_t ev_retire;
    // int8 all-pairs adaptive dispatch (mv_match_allpairs_i8_dev): pinned count of the pairs the
    // last measuring call handed back, that call's batch, calls so far
    int *i8_count_host;
    int i8_meas_batch;
    unsigned i8_calls;
    bool i8_prefer_m;  // the last landed measurement: most pairs handed back
    // k_q8t_match (persistent): the device word its workgroups draw pairs from -- allocated and
    // zeroed with the context, zeroed again by the kernel that follows each launch; not in `scratch`,
    // which other entry points write -- and the device's CU count (read once, never under a capture)
    int *q8t_ticket;
    int cu_count;
};

namespace mv {

void set_error(int status, const char *fmt, ...);
int set_status(int status);

// true while `s` is captured into a graph (or the query is refused: see mv_context.hip)
int capture_state(hipStream_t s, bool *cap);  // MV_OK + *cap, or MV_ERR_HIP (reported)
// Grow (never shrink) `b` to at least `bytes`, rounded up to 1 MiB.  Growing quiesces the context
// and frees the old buffer; when the quiesce fails its status is returned and the old buffer stays.
// A failed allocation leaves the buffer empty.  `what` names the buffer in the error message.
int grow(mv_context *ctx, mv_buffer &b, size_t bytes, const char *what);
// the context scratch / staging buffer of at least `bytes`; nullptr on failure
void *scratch(mv_context *ctx, size_t bytes);
void *stage(mv_context *ctx, size_t bytes);
// Carve `layout` (a callable on a Carve &, written once) out of the context scratch / staging
// buffer: a measuring pass sizes the buffer, a second pass on its base places the arrays.
// false: the buffer could not be had (out of memory)
template <class F>
bool carve(void *(*buffer)(mv_context *, size_t), mv_context *ctx, F layout) {
    Carve need{nullptr};
    layout(need);
    Carve c{static_cast<char *>(buffer(ctx, need.bytes()))};
    if (c.base) layout(c);
    return c.base != nullptr;
}

// an array of a call (k_mapcorr.hip, k_mapcull.hip): no array that is written may overlap another one
struct Span {
    const void *p;  // nullptr: an optional array that was not given
    size_t bytes;
    bool written;
};

inline bool no_overlap(std::initializer_list<Span> spans) {
    for (const Span *a = spans.begin(); a != spans.end(); a++)
        for (const Span *b = a + 1; b != spans.end(); b++) {
            if (!(a->written || b->written) || !a->p || !b->p) continue;
            const uintptr_t a0 = (uintptr_t)a->p, b0 = (uintptr_t)b->p;
            if (a0 < b0 + b->bytes && b0 < a0 + a->bytes) return false;
        }
    return true;
}

// Wait for every stream this context has issued work on (its own stream -- which waits on every
// stream the context left, via ev_retire --, the current stream and the staging stream) -- before
// a context buffer is freed; other contexts and threads are not blocked (no device-wide
// synchronisation unless a synchronisation itself fails).
int quiesce(mv_context *ctx);
// bytes of one staged frame-1 image (ap_image / ap_image2) under `screen` (mv_allpairs.hip)
size_t ap_image_bytes(int screen, int batch, int cap);

// Kernel profiler (mv_profile_* in maveric_hip.h): when enabled, launchers
// bracket each kernel with hipEventRecord on the launch stream -- no sync.
bool prof_on();
void prof_begin(hipStream_t s, const char *kernel);
void prof_end(hipStream_t s);

}  // namespace mv

#define MV_PROF_BEGIN(s, name) \
    do {                       \
        if (mv::prof_on()) mv::prof_begin((s), (name)); \
    } while (0)
#define MV_PROF_END(s)         \
    do {                       \
        if (mv::prof_on()) mv::prof_end(s); \
    } while (0)

#define MV_HIP_TRY(expr)                                                                   \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            mv::set_error(MV_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #expr,           \
                          hipGetErrorString(_e));                                          \
            return MV_ERR_HIP;                                                             \
        }                                                                                  \
    } while (0)

// The one launch form: the profiler bracket under `name` (nullptr: none), the launch, and the
// launch check, which returns MV_ERR_HIP from the enclosing function with the launch site's
// file:line.  A template kernel goes in parentheses, as for hipLaunchKernelGGL.
#define MV_LAUNCH(name, kernel, grid, block, lds_bytes, stream, ...)                       \
    do {                                                                                   \
        const char *_name = (name);                                                        \
        if (_name) MV_PROF_BEGIN((stream), _name);                                         \
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, __VA_ARGS__);           \
        if (_name) MV_PROF_END(stream);                                                    \
        MV_HIP_TRY(hipGetLastError());                                                     \
    } while (0)

#define MV_REQUIRE(cond)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            mv::set_error(MV_ERR_INVALID_ARG, "%s:%d invalid argument: %s", __FILE__,      \
                          __LINE__, #cond);                                                \
            return MV_ERR_INVALID_ARG;                                                     \
        }                                                                                  \
    } while (0)

// ---------------------------------------------------------------------------
// Launchers implemented in the kernel translation units (stream-ordered).
// ---------------------------------------------------------------------------
namespace mv {
int launch_softmax(hipStream_t s, int batch, int cells, const float *scales, const int8_t *semi,
                   int *max_idx, float *probs, int *num_valid);
int launch_top_n_select(hipStream_t s, int batch, int cells, const int *max_idx, const float *probs, int N,
                        int cap, int *num_sel, int *patches, int *indices, float *sel_probs, int *status);
size_t allpairs_f32_image_bytes(int batch, int cap);  // the fp16 image of k_ap_split
int launch_allpairs_f32_prepare(hipStream_t s, void *scratch, int batch, int cap, const int *n1,
                                const float *desc1);
int launch_allpairs_f32_match(hipStream_t s, void *scratch, int batch, int cap, const int *n0, const int *n1,
                              const float *desc0, const float *desc1, double thresh, int *match_idx,
                              float *match_score, int dmode = 0);
size_t allpairs_q8_scratch_bytes(int batch, int cap);
int launch_allpairs_q8_prepare(hipStream_t s, void *scratch, int batch, int cap, const int *n1,
                               const float *desc1);
int launch_allpairs_q8_match(hipStream_t s, void *scratch, int batch, int cap, const int *n0, const int *n1,
                             const float *desc0, const float *desc1, double thresh, int *match_idx,
                             float *match_score, int dmode = 0);
// sequence mode: frames 0 .. frames-1, pair b = (b, b + 1); every frame quantised once
int launch_allpairs_q8_sequence(hipStream_t s, void *scratch, int frames, int cap, const int *n, const float *desc,
                                double thresh, int *match_idx, float *match_score, bool prepared = false,
                                void *next_scratch = nullptr, int next_frames = 0, int next_cap = 0,
                                const int *next_n = nullptr, const float *next_desc = nullptr);
// the match plus the next batch's frame-1 staging into next_scratch, in one launch
int launch_allpairs_q8_match_prepare(hipStream_t s, void *scratch, int batch, int cap, const int *n0, const int *n1,
                                     const float *desc0, const float *desc1, double thresh, int *match_idx,
                                     float *match_score, int dmode, void *next_scratch, int next_batch,
                                     int next_cap, const int *next_n1, const float *next_desc1);
// the single-pass int8 screen (k_allpairs_direct.hip): no scratch, frame 1 quantised in-kernel
// only: per-pair flags -- the workgroups of pairs whose flag is 0 exit at once (k_q8t_match's
// hand-backs); null: every pair
int launch_allpairs_q8d_match(hipStream_t s, int batch, int cap, const int *n0, const int *n1, const float *desc0,
                              const float *desc1, double thresh, int *match_idx, float *match_score, int dmode = 0,
                              const int *only = nullptr);
// the pair-per-workgroup transposed kernel (k_allpairs_direct.hip; persistent, `cus` workgroups
// drawing pairs from the context's `ticket` word), k_q8d_match for its hand-backs;
// scratch >= allpairs_q8t_scratch_bytes(batch)
bool allpairs_q8t_applies(int cap, int dmode);
size_t allpairs_q8t_scratch_bytes(int batch);
int launch_allpairs_q8t_match(hipStream_t s, void *scratch, int *ticket, int cus, int batch, int cap, const int *n0,
                              const int *n1, const float *desc0, const float *desc1, double thresh, int *match_idx,
                              float *match_score);
size_t allpairs_i8_scratch_bytes(int batch, int cap);
int launch_allpairs_i8(hipStream_t s, void *scratch, int batch, int cap, const int *n0, const int *n1,
                       const int8_t *desc0, const int8_t *desc1, int *match_idx, int *match_dot, bool direct = false,
                       int *count_host = nullptr);
// the batched pose by p->semantics (k_pose.hip); as-intended: k_pose_ransac (k_pose_intended.hip)
int launch_pose(hipStream_t s, const mv_pose_params *p, int batch, int cap, const int *n, const float *pts0,
                const float *pts1, const int *match_idx, const float *kp1, float *T, int *num_matches,
                int *num_inliers, int *status);
int launch_intended_pose(hipStream_t s, const mv_pose_params *p, int batch, int cap, const int *n, const float *pts0,
                         const float *pts1, const int *match_idx, const float *kp1, float *T, int *num_matches,
                         int *num_inliers, int *status);
int launch_ransac_stub(hipStream_t s, int n, const float *pts1, const float *pts2, float thresh, float *E,
                       int *inliers, int *num_inliers);
int launch_recover_pose(hipStream_t s, const float *E, float *R1, float *R2, float *t);
int launch_svd3(hipStream_t s, const float *A, float *U, float *S, float *V);
}  // namespace mv
