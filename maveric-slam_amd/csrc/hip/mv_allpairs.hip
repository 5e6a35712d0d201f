// mv_allpairs.hip -- host side of the fp32 all-pairs match: the seven entry points
//   mv_match_allpairs_f32_dev, ..._prepare_dev, ..._run_dev, ..._run_prepare_dev,
//   mv_match_two_way_f32_dev, mv_match_sequence_f32_dev, ..._sequence_f32_run_prepare_dev
// dispatching over the context's screen: the one-pass int8 kernels (k_allpairs_direct.hip, the
// default: frame 1 read as fp32, nothing staged), the staged int8 kernels (k_allpairs_q8.hip) and
// the fp16 kernels (k_allpairs_f32.hip), the last two matching against an image of frame 1.
// The prepared batch (mv_context::prep) and the two images (ap_image, ap_image2) are handled here
// only; mv_context_reserve grows the images ahead of time.
#include <utility>

#include "mv_internal.hpp"

namespace mv {
// one staged image under `screen`: fp16 (516 B per row) or int8 (268 B per row)
size_t ap_image_bytes(int screen, int batch, int cap) {
    return screen == MV_SCREEN_F16 ? allpairs_f32_image_bytes(batch, cap) : allpairs_q8_scratch_bytes(batch, cap);
}
}  // namespace mv

namespace {
// the first image, grown to `bytes`: a prepared frame 1 lived in a buffer that was replaced
int ap_grow_image(mv_context *ctx, size_t bytes) {
    const size_t was = ctx->ap_image.bytes;
    const int st = mv::grow(ctx, ctx->ap_image, bytes, "all-pairs scratch");
    if (was && ctx->ap_image.bytes != was) ctx->prep.invalidate();
    return st;
}
// the second image (run_prepare's staging target)
int ap_grow_image2(mv_context *ctx, size_t bytes) {
    return mv::grow(ctx, ctx->ap_image2, bytes, "all-pairs scratch");
}
// the staging stream and its two events, created on first use
int ap_aux_stream(mv_context *ctx) {
    if (ctx->aux_stream) return MV_OK;
    MV_HIP_TRY(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
    MV_HIP_TRY(hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
    MV_HIP_TRY(hipEventCreateWithFlags(&ctx->ev_prep, hipEventDisableTiming));
    return MV_OK;
}
// the context stream waits for a staging still in flight on the staging stream
int ap_wait_staging(mv_context *ctx) {
    if (ctx->aux_stream) MV_HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_prep, 0));
    return MV_OK;
}
// run_prepare staged the next batch into the second image: it becomes the prepared one
void ap_swap_prepared(mv_context *ctx, int batch, int cap, const int *n1, const float *desc1) {
    std::swap(ctx->ap_image, ctx->ap_image2);
    ctx->prep.record(batch, cap, n1, desc1, ctx->prep.screen, true);
}

// staging of frame 1 for the screens that match against an image (fp16, staged int8; the
// default int8 screen stages only for sequence mode, which reuses the images)
int ap_prepare(int screen, hipStream_t s, void *scr, int batch, int cap, const int *n1, const float *desc1) {
    return screen == MV_SCREEN_F16 ? mv::launch_allpairs_f32_prepare(s, scr, batch, cap, n1, desc1)
                                   : mv::launch_allpairs_q8_prepare(s, scr, batch, cap, n1, desc1);
}
// the match; MV_SCREEN_I8 reads both fp32 frames directly (no image, scr unused)
int ap_match(mv_context *ctx, int screen, hipStream_t s, void *scr, int batch, int cap, const int *n0, const int *n1,
             const float *desc0, const float *desc1, double thresh, int *match_idx, float *match_score,
             int dmode = 0) {
    if (screen == MV_SCREEN_I8) {
        if (mv::allpairs_q8t_applies(cap, dmode)) {
            void *fl = mv::scratch(ctx, mv::allpairs_q8t_scratch_bytes(batch));
            if (!fl) return MV_ERR_OUT_OF_MEMORY;
            return mv::launch_allpairs_q8t_match(s, fl, ctx->q8t_ticket, ctx->cu_count, batch, cap, n0, n1, desc0, desc1, thresh, match_idx,
                                                 match_score);
        }
        return mv::launch_allpairs_q8d_match(s, batch, cap, n0, n1, desc0, desc1, thresh, match_idx, match_score,
                                             dmode);
    }
    return screen == MV_SCREEN_F16
               ? mv::launch_allpairs_f32_match(s, scr, batch, cap, n0, n1, desc0, desc1, thresh, match_idx,
                                               match_score, dmode)
               : mv::launch_allpairs_q8_match(s, scr, batch, cap, n0, n1, desc0, desc1, thresh, match_idx,
                                              match_score, dmode);
}
// a one-shot call on an image screen: the first image for `batch` x `cap`, about to be overwritten
// (so nothing stays prepared), once a staging in flight has finished with it
int ap_claim_image(mv_context *ctx, int batch, int cap) {
    const int st = ap_grow_image(ctx, mv::ap_image_bytes(ctx->ap_screen, batch, cap));
    if (st != MV_OK) return st;
    ctx->prep.invalidate();
    return ap_wait_staging(ctx);
}
}  // namespace

extern "C" int mv_match_allpairs_f32_dev(mv_context *ctx, int batch, int cap, const int *n0, const int *n1,
                                         const float *desc0, const float *desc1, double thresh, int *match_idx,
                                         float *match_score) {
    MV_REQUIRE(ctx != nullptr && batch > 0 && cap > 0);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->ap_screen == MV_SCREEN_I8)  // one pass, no image
        return ap_match(ctx, ctx->ap_screen, ctx->stream, nullptr, batch, cap, n0, n1, desc0, desc1, thresh, match_idx,
                        match_score);
    int st = ap_claim_image(ctx, batch, cap);
    if (st == MV_OK) st = ap_prepare(ctx->ap_screen, ctx->stream, ctx->ap_image.p, batch, cap, n1, desc1);
    if (st != MV_OK) return st;
    return ap_match(ctx, ctx->ap_screen, ctx->stream, ctx->ap_image.p, batch, cap, n0, n1, desc0, desc1, thresh,
                    match_idx, match_score);
}

extern "C" int mv_match_allpairs_f32_prepare_dev(mv_context *ctx, int batch, int cap, const int *n1,
                                                 const float *desc1) {
    MV_REQUIRE(ctx != nullptr && batch > 0 && cap > 0 && n1 && desc1);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->ap_screen == MV_SCREEN_I8) {  // the one-pass match reads frame 1 itself: record only
        ctx->prep.record(batch, cap, n1, desc1, ctx->ap_screen, false);  // sequence mode stages on first use
        return mv::set_status(MV_OK);
    }
    int st = ap_grow_image(ctx, mv::ap_image_bytes(ctx->ap_screen, batch, cap));
    if (st == MV_OK) st = ap_aux_stream(ctx);
    if (st != MV_OK) return st;
    // inputs (and the previous run's use of the scratch) as of this call on the context stream
    MV_HIP_TRY(hipEventRecord(ctx->ev_in, ctx->stream));
    MV_HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_in, 0));
    st = ap_prepare(ctx->ap_screen, ctx->aux_stream, ctx->ap_image.p, batch, cap, n1, desc1);
    if (st != MV_OK) return st;
    MV_HIP_TRY(hipEventRecord(ctx->ev_prep, ctx->aux_stream));
    ctx->prep.record(batch, cap, n1, desc1, ctx->ap_screen, true);
    return MV_OK;
}

extern "C" int mv_match_allpairs_f32_run_dev(mv_context *ctx, int batch, int cap, const int *n0, const int *n1,
                                             const float *desc0, const float *desc1, double thresh, int *match_idx,
                                             float *match_score) {
    MV_REQUIRE(ctx != nullptr);
    if (!ctx->prep.matches(batch, cap, n1, desc1) || ctx->prep.screen != ctx->ap_screen) {
        mv::set_error(MV_ERR_INVALID_ARG, "mv_match_allpairs_f32_run_dev: no matching prepare for this batch");
        return MV_ERR_INVALID_ARG;
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->prep.staged) {
        const int st = ap_wait_staging(ctx);
        if (st != MV_OK) return st;
    }
    return ap_match(ctx, ctx->ap_screen, ctx->stream, ctx->ap_image.p, batch, cap, n0, n1, desc0, desc1, thresh,
                    match_idx, match_score);
}

extern "C" int mv_match_allpairs_f32_run_prepare_dev(mv_context *ctx, int batch, int cap, const int *n0,
                                                     const int *n1, const float *desc0, const float *desc1,
                                                     double thresh, int *match_idx, float *match_score,
                                                     int next_batch, int next_cap, const int *next_n1,
                                                     const float *next_desc1) {
    MV_REQUIRE(ctx != nullptr && next_batch > 0 && next_cap > 0 && next_n1 && next_desc1);
    if (!ctx->prep.matches(batch, cap, n1, desc1) || ctx->prep.screen != ctx->ap_screen) {
        mv::set_error(MV_ERR_INVALID_ARG, "mv_match_allpairs_f32_run_prepare_dev: no matching prepare for this batch");
        return MV_ERR_INVALID_ARG;
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->ap_screen == MV_SCREEN_I8) {  // one pass: nothing to stage for the next batch
        const int st = ap_match(ctx, ctx->ap_screen, ctx->stream, nullptr, batch, cap, n0, n1, desc0, desc1, thresh,
                                match_idx, match_score);
        if (st != MV_OK) return st;
        // recorded, not staged (sequence mode stages on first use)
        ctx->prep.record(next_batch, next_cap, next_n1, next_desc1, ctx->prep.screen, false);
        return mv::set_status(MV_OK);
    }
    int st = ap_grow_image2(ctx, mv::ap_image_bytes(ctx->ap_screen, next_batch, next_cap));
    if (st == MV_OK) st = ap_wait_staging(ctx);
    if (st != MV_OK) return st;
    if (ctx->ap_screen == MV_SCREEN_I8_STAGED) {
        st = mv::launch_allpairs_q8_match_prepare(ctx->stream, ctx->ap_image.p, batch, cap, n0, n1, desc0, desc1,
                                                  thresh, match_idx, match_score, 0, ctx->ap_image2.p, next_batch,
                                                  next_cap, next_n1, next_desc1);
    } else {  // the fp16 screen: the two kernels in stream order
        st = ap_match(ctx, ctx->ap_screen, ctx->stream, ctx->ap_image.p, batch, cap, n0, n1, desc0, desc1, thresh,
                      match_idx, match_score);
        if (st == MV_OK)
            st = ap_prepare(ctx->ap_screen, ctx->stream, ctx->ap_image2.p, next_batch, next_cap, next_n1, next_desc1);
    }
    if (st != MV_OK) return st;
    ap_swap_prepared(ctx, next_batch, next_cap, next_n1, next_desc1);  // the next batch is now the prepared one
    return mv::set_status(MV_OK);
}

namespace {
// nn_match_two_way's keep (pairwise_pnp.py:307-313): dist < nn_thresh (float32 compare) and
// the reverse argmin of the match is the row itself
__global__ __launch_bounds__(256) void k_two_way_keep(long total, int cap, const int *__restrict__ n0v,
                                                      const int *__restrict__ n1v, const int *__restrict__ ridx,
                                                      float nn_thresh, int *__restrict__ fidx,
                                                      float *__restrict__ fdist, int keep_dist) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const long b = q / cap;
    const int i = (int)(q % cap);
    const int n0 = min(max(n0v[b], 0), cap), n1 = min(max(n1v[b], 0), cap);
    const int j = fidx[q];
    const bool keep = i < n0 && j >= 0 && j < n1 && fdist[q] < nn_thresh && ridx[b * cap + j] == i;
    fidx[q] = keep ? j : -1;
    if (keep_dist && !keep) fdist[q] = 0.f;
}
}  // namespace

extern "C" int mv_match_two_way_f32_dev(mv_context *ctx, int batch, int cap, const int *n0, const int *n1,
                                        const float *desc0, const float *desc1, double nn_thresh, int *match_idx,
                                        float *match_dist) {
    MV_REQUIRE(ctx != nullptr && batch > 0 && cap > 0 && n0 && n1 && desc0 && desc1 && match_idx);
    if (!(nn_thresh >= 0.0)) {
        mv::set_error(MV_ERR_INVALID_ARG, "nn_match_two_way: nn_thresh should be non-negative");
        return MV_ERR_INVALID_ARG;
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    const int sc = ctx->ap_screen;
    void *scr = nullptr;
    if (sc != MV_SCREEN_I8) {  // the image screens stage each direction
        const int st = ap_claim_image(ctx, batch, cap);
        if (st != MV_OK) return st;
        scr = ctx->ap_image.p;
    }
    int *ridx;
    float *tdist;  // the distances, when the caller keeps none
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) {
            ridx = c.take<int>((size_t)batch * cap);
            tdist = c.take<float>((size_t)batch * cap);
        }))
        return MV_ERR_OUT_OF_MEMORY;
    float *fdist = match_dist ? match_dist : tdist;
    hipStream_t s = ctx->stream;
    // forward: rows of frame 0 against frame 1 (argmin distance + its exact distance)
    int st = sc == MV_SCREEN_I8 ? MV_OK : ap_prepare(sc, s, scr, batch, cap, n1, desc1);
    if (st == MV_OK) st = ap_match(ctx, sc, s, scr, batch, cap, n0, n1, desc0, desc1, 0.0, match_idx, fdist, 1);
    // reverse: rows of frame 1 against frame 0 (indices only)
    if (st == MV_OK && sc != MV_SCREEN_I8) st = ap_prepare(sc, s, scr, batch, cap, n0, desc0);
    if (st == MV_OK) st = ap_match(ctx, sc, s, scr, batch, cap, n1, n0, desc1, desc0, 0.0, ridx, nullptr, 1);
    if (st != MV_OK) return st;
    const long total = (long)batch * cap;
    MV_LAUNCH(nullptr, k_two_way_keep, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, cap, n0, n1, ridx,
              (float)nn_thresh, match_idx, fdist, match_dist ? 1 : 0);
    return mv::set_status(MV_OK);
}

namespace {
// Sequence mode on the default screen (cap <= 1024): k_q8t_match over the F - 1 pairs (frame b,
// frame b + 1) addressed in place -- desc0 = desc, desc1 = desc + one frame, n0 = n, n1 = n + 1 -- a
// whole pair per workgroup, each frame read once as frame 1 and once as frame 0 (the staged int8
// images of k_q8_match<AI8> read 24 % fewer bytes but run the older, slower sweep: 4.0 ms per 8192
// pairs against the one-pass kernel's 3.5)
bool seq_one_pass(const mv_context *ctx, int cap) {
    return ctx->ap_screen == MV_SCREEN_I8 && mv::allpairs_q8t_applies(cap, 0);
}
int seq_one_pass_run(mv_context *ctx, int frames, int cap, const int *n, const float *desc, double thresh,
                     int *match_idx, float *match_score) {
    void *fl = mv::scratch(ctx, mv::allpairs_q8t_scratch_bytes(frames - 1));
    if (!fl) return MV_ERR_OUT_OF_MEMORY;
    return mv::launch_allpairs_q8t_match(ctx->stream, fl, ctx->q8t_ticket, ctx->cu_count, frames - 1, cap, n, n + 1,
                                         desc, desc + (size_t)cap * 256, thresh, match_idx, match_score);
}
}  // namespace

extern "C" int mv_match_sequence_f32_dev(mv_context *ctx, int frames, int cap, const int *n, const float *desc,
                                         double thresh, int *match_idx, float *match_score) {
    MV_REQUIRE(ctx != nullptr && frames >= 2 && cap > 0 && n && desc && match_idx);
    if (ctx->ap_screen == MV_SCREEN_F16) {
        mv::set_error(MV_ERR_INVALID_ARG, "mv_match_sequence_f32_dev: the int8 screens only");
        return MV_ERR_INVALID_ARG;
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    int st;
    if (seq_one_pass(ctx, cap)) {  // in place: a prepared batch stays prepared
        st = seq_one_pass_run(ctx, frames, cap, n, desc, thresh, match_idx, match_score);
    } else {
        st = ap_claim_image(ctx, frames, cap);
        if (st == MV_OK)
            st = mv::launch_allpairs_q8_sequence(ctx->stream, ctx->ap_image.p, frames, cap, n, desc, thresh, match_idx,
                                                 match_score);
    }
    return st != MV_OK ? st : mv::set_status(MV_OK);
}

extern "C" int mv_match_sequence_f32_run_prepare_dev(mv_context *ctx, int frames, int cap, const int *n,
                                                     const float *desc, double thresh, int *match_idx,
                                                     float *match_score, int next_frames, int next_cap,
                                                     const int *next_n, const float *next_desc) {
    MV_REQUIRE(ctx != nullptr && frames >= 2 && next_frames >= 2 && next_cap > 0 && next_n && next_desc);
    // either int8 screen may have prepared the frames (the looser rule: only fp16 is excluded)
    if (!ctx->prep.matches(frames, cap, n, desc) || ctx->ap_screen == MV_SCREEN_F16 ||
        ctx->prep.screen == MV_SCREEN_F16) {
        mv::set_error(MV_ERR_INVALID_ARG,
                      "mv_match_sequence_f32_run_prepare_dev: no matching prepare for these frames (int8 screen)");
        return MV_ERR_INVALID_ARG;
    }
    MV_HIP_TRY(hipSetDevice(ctx->device));
    if (seq_one_pass(ctx, cap)) {  // nothing staged: match this chunk in place, record the next one
        const int st = seq_one_pass_run(ctx, frames, cap, n, desc, thresh, match_idx, match_score);
        if (st != MV_OK) return st;
        ctx->prep.record(next_frames, next_cap, next_n, next_desc, ctx->prep.screen, false);
        return mv::set_status(MV_OK);
    }
    int st;
    if (!ctx->prep.staged) {  // recorded by the one-pass screen's prepare: stage the images now
        st = ap_grow_image(ctx, mv::ap_image_bytes(ctx->ap_screen, frames, cap));
        if (st == MV_OK) st = ap_wait_staging(ctx);
        if (st == MV_OK) st = ap_prepare(ctx->ap_screen, ctx->stream, ctx->ap_image.p, frames, cap, n, desc);
        if (st != MV_OK) return st;
        ctx->prep.staged = true;
    }
    st = ap_grow_image2(ctx, mv::ap_image_bytes(ctx->ap_screen, next_frames, next_cap));
    if (st == MV_OK) st = ap_wait_staging(ctx);
    if (st == MV_OK)
        st = mv::launch_allpairs_q8_sequence(ctx->stream, ctx->ap_image.p, frames, cap, n, desc, thresh, match_idx,
                                             match_score, true, ctx->ap_image2.p, next_frames, next_cap, next_n,
                                             next_desc);
    if (st != MV_OK) return st;
    ap_swap_prepared(ctx, next_frames, next_cap, next_n, next_desc);
    return mv::set_status(MV_OK);
}
