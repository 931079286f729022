/* engine_track_draw_frames.c - consecutive camera frames in; every frame comes out with its detections painted in the colour of
 * their track, a text label each, and a bird's-eye panel of the tracker's table with fading trails - from plain C (no Python,
 * no torch, no image library): engine_track_frames.c plus one rtm3d_records_draw_tracks call per step.
 *
 *   engine_track_draw_frames ENGINE PREFIX FRAMES.bin [FRAMES.bin ...]
 *
 * ENGINE      an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * FRAMES.bin  one per time step, in order, each in the format of engine_detect_frames.c: int32 B (the engine's batch); per
 *             frame int32 h, w and h * w * 3 bytes; B x 9 float64 camera intrinsics; float32 mean[3], std[3]; int32 resize_to.
 *             Batch index b of every file is the next frame of stream b.
 * PREFIX      output: per step f = 0, 1, .. PREFIX<f>_frame.ppm (frame 0, painted) and PREFIX<f>_panel.ppm (the 400 x 400 panel
 *             of stream 0 at 0.2 m per pixel, camera at the bottom centre), binary PPM (P6), channels as in the input
 *
 * Per file, on one stream: rtm3d_engine_detect_frames, rtm3d_tracks_update (default parameters, 128 track slots, dt = 1, no ego
 * motion), rtm3d_records_draw_tracks with the defaults plus: thickness 2, the label layer (id, class, score; font scale 2; the
 * KITTI class names), the track-driven panel with bev_fade 200.  The panels start black and are passed again every step.
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define TRACK_SLOTS 128
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_track_draw_frames: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_track_draw_frames: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)
#define READ(ptr, size, count) do { if (fread((ptr), (size), (count), in) != (size_t)(count)) { \
    fprintf(stderr, "engine_track_draw_frames: %s is truncated\n", path); goto done; } } while (0)

/* one FRAMES.bin: the frames go to fresh device buffers d_imgs[b] (the caller frees them), sizes to h_hw, intrinsics to h_K */
static int load_frames(const char* path, int B, uint8_t** d_imgs, int* h_hw, double* h_K, rtm3d_frame_params* params) {
    FILE* in = fopen(path, "rb");
    uint8_t* h_img = NULL;
    int32_t n = 0, resize_to;
    int b, rc = 1;
    if (!in) { fprintf(stderr, "engine_track_draw_frames: cannot open %s\n", path); return 1; }
    READ(&n, sizeof n, 1);
    if (n != B) { fprintf(stderr, "engine_track_draw_frames: %s holds %d frames, the engine runs batches of %d\n", path, (int)n, B); goto done; }
    for (b = 0; b < B; ++b) {
        int32_t hw[2];
        size_t bytes;
        READ(hw, sizeof(int32_t), 2);
        if (hw[0] < 1 || hw[1] < 1 || hw[0] > 16384 || hw[1] > 16384) {
            fprintf(stderr, "engine_track_draw_frames: %s: frame %d has size %d x %d\n", path, b, (int)hw[0], (int)hw[1]);
            goto done;
        }
        h_hw[2 * b] = hw[0]; h_hw[2 * b + 1] = hw[1];
        bytes = (size_t)hw[0] * hw[1] * 3;
        free(h_img);
        h_img = (uint8_t*)malloc(bytes);
        if (!h_img) { fprintf(stderr, "engine_track_draw_frames: out of host memory\n"); goto done; }
        READ(h_img, 1, bytes);
        HIP_OK(hipMalloc((void**)&d_imgs[b], bytes));
        HIP_OK(hipMemcpy(d_imgs[b], h_img, bytes, hipMemcpyHostToDevice));
    }
    READ(h_K, sizeof(double), (size_t)B * 9);
    READ(params->mean, sizeof(float), 3);
    READ(params->std, sizeof(float), 3);
    READ(&resize_to, sizeof resize_to, 1);
    params->resize_to = resize_to;
    rc = 0;
done:
    free(h_img);
    fclose(in);
    return rc;
}

#define BEV_SIDE 400

static int write_ppm(const char* prefix, int step, const char* what, const uint8_t* src, int h, int w) {
    char path[4096];
    FILE* f;
    const size_t bytes = (size_t)h * w * 3;
    if (snprintf(path, sizeof path, "%s%d_%s.ppm", prefix, step, what) >= (int)sizeof path) { fprintf(stderr, "engine_track_draw_frames: PREFIX is too long\n"); return 1; }
    f = fopen(path, "wb");
    if (!f || fprintf(f, "P6\n%d %d\n255\n", w, h) < 0 || fwrite(src, 1, bytes, f) != bytes) {
        fprintf(stderr, "engine_track_draw_frames: cannot write %s\n", path);
        if (f) fclose(f);
        return 1;
    }
    return fclose(f) != 0;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s ENGINE PREFIX FRAMES.bin [FRAMES.bin ...]\n", argv[0]);
        return 2;
    }
    static const char* const names[3] = {"Car", "Pedestr", "Cyclist"};
    int rc = 1, b, f, n_files = argc - 3, B, params_set = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params fparams;
    rtm3d_track_params tparams;
    rtm3d_draw_tracks_params dparams;
    int* h_hw = NULL;
    uint8_t **d_imgs = NULL, *d_bev = NULL, *h_out = NULL;
    float* d_rec = NULL;
    double *h_K = NULL, *d_K = NULL, *d_state = NULL;
    int32_t* d_ids = NULL;
    void *d_ws = NULL, *d_tws = NULL;
    hipStream_t stream = NULL;
    size_t n_slots, bev_bytes = (size_t)BEV_SIDE * BEV_SIDE * 3;

    if (rtm3d_engine_load(argv[1], 0, &ctx, &info) != 0) {
        fprintf(stderr, "engine_track_draw_frames: %s\n", rtm3d_last_error());
        return 1;
    }
    B = info.B;
    n_slots = (size_t)B * info.topk;
    h_hw = (int*)malloc((size_t)B * 2 * sizeof(int));
    d_imgs = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)B * 9 * sizeof(double));
    if (!h_hw || !d_imgs || !h_K) { fprintf(stderr, "engine_track_draw_frames: out of host memory\n"); goto done; }

    RT_OK(rtm3d_track_default_params(&tparams));
    RT_OK(rtm3d_draw_tracks_default_params(&dparams));
    dparams.base.layers |= RTM3D_DRAW_LABEL | RTM3D_DRAW_TRACK_BEV;
    dparams.base.thickness = 2;
    dparams.base.bev_h = BEV_SIDE; dparams.base.bev_w = BEV_SIDE; dparams.base.bev_m_per_px = 0.2;
    dparams.label_fields = 1 | 2 | 4;
    dparams.font_scale = 2;
    dparams.bev_fade = 200;
    memset(dparams.names, 0, sizeof dparams.names);
    for (b = 0; b < 3; ++b) memcpy(dparams.names[b], names[b], strlen(names[b]));            /* at most 7 characters, NUL after them */
    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_ids, n_slots * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_bev, (size_t)B * bev_bytes));
    HIP_OK(hipMalloc((void**)&d_state, rtm3d_tracks_state_bytes(B, TRACK_SLOTS)));
    HIP_OK(hipMalloc(&d_tws, rtm3d_tracks_workspace_bytes(B, info.topk, TRACK_SLOTS)));
    HIP_OK(hipMemsetAsync(d_state, 0, rtm3d_tracks_state_bytes(B, TRACK_SLOTS), stream));      /* all streams empty */
    HIP_OK(hipMemsetAsync(d_bev, 0, (size_t)B * bev_bytes, stream));                           /* the panels are the caller's: black */
    for (f = 0; f < n_files; ++f) {
        size_t bytes;
        if (load_frames(argv[3 + f], B, d_imgs, h_hw, h_K, &fparams) != 0) goto done;
        if (!params_set) {
            RT_OK(rtm3d_engine_set_frame_params(ctx, &fparams));
            HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
            params_set = 1;
        }
        HIP_OK(hipMemcpyAsync(d_K, h_K, (size_t)B * 9 * sizeof(double), hipMemcpyHostToDevice, stream));
        RT_OK(rtm3d_engine_detect_frames(ctx, stream, (const uint8_t* const*)d_imgs, h_hw, d_K, d_rec, NULL, d_ws));
        RT_OK(rtm3d_tracks_update(stream, B, info.topk, TRACK_SLOTS, d_rec, 1.0, NULL, &tparams, d_state, d_ids, d_tws));
        /* the one new call: the frames and the panels of this step, behind the tracker on the same stream */
        RT_OK(rtm3d_records_draw_tracks(stream, B, info.topk, d_rec, d_ids, TRACK_SLOTS, d_state, (uint8_t* const*)d_imgs, h_hw, d_K, &dparams, d_bev));
        HIP_OK(hipStreamSynchronize(stream));
        bytes = (size_t)h_hw[0] * h_hw[1] * 3;
        free(h_out);
        h_out = (uint8_t*)malloc(bytes > bev_bytes ? bytes : bev_bytes);
        if (!h_out) { fprintf(stderr, "engine_track_draw_frames: out of host memory\n"); goto done; }
        HIP_OK(hipMemcpy(h_out, d_imgs[0], bytes, hipMemcpyDeviceToHost));
        if (write_ppm(argv[2], f, "frame", h_out, h_hw[0], h_hw[1])) goto done;
        HIP_OK(hipMemcpy(h_out, d_bev, bev_bytes, hipMemcpyDeviceToHost));
        if (write_ppm(argv[2], f, "panel", h_out, BEV_SIDE, BEV_SIDE)) goto done;
        printf("engine_track_draw_frames: %s: frame 0 %dx%d and its panel written\n", argv[3 + f], h_hw[0], h_hw[1]);
        for (b = 0; b < B; ++b) { (void)hipFree(d_imgs[b]); d_imgs[b] = NULL; }
    }
    rc = 0;
done:
    if (d_tws) (void)hipFree(d_tws);
    if (d_ws) (void)hipFree(d_ws);
    if (d_state) (void)hipFree(d_state);
    if (d_bev) (void)hipFree(d_bev);
    if (d_ids) (void)hipFree(d_ids);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_imgs) for (b = 0; b < B; ++b) if (d_imgs[b]) (void)hipFree(d_imgs[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(d_imgs); free(h_hw); free(h_K); free(h_out);
    return rc;
}
