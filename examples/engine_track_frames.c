/* engine_track_frames.c - consecutive camera frames in, a track id per kept 3D box out, from plain C (no Python, no torch).
 *
 *   engine_track_frames ENGINE IDS.i32 FRAMES.bin [FRAMES.bin ...] [optimal]
 *
 * ENGINE      an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * FRAMES.bin  one per time step, in order, each in the format of engine_detect_frames.c: int32 B (the engine's batch); per
 *             frame int32 h, w and h * w * 3 bytes; B x 9 float64 camera intrinsics; float32 mean[3], std[3]; int32 resize_to.
 *             Batch index b of every file is the next frame of stream b.
 * IDS.i32     output: per file B x topk raw int32, one per record slot: +id confirmed track, -id tentative, 0 not tracked
 *
 * Per file, on one stream and without a synchronisation in between: rtm3d_engine_detect_frames, then rtm3d_tracks_update with
 * the default parameters (rtm3d_track_default_params), 128 track slots per stream, dt = 1, no ego motion.  A trailing word
 * "optimal" runs rtm3d_tracks_update_assign with RTM3D_TRACK_ASSIGN_OPTIMAL instead (the optimal assignment, not the greedy match).
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define TRACK_SLOTS 128
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_track_frames: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_track_frames: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)
#define READ(ptr, size, count) do { if (fread((ptr), (size), (count), in) != (size_t)(count)) { \
    fprintf(stderr, "engine_track_frames: %s is truncated\n", path); goto done; } } while (0)

/* one FRAMES.bin: the frames go to fresh device buffers d_imgs[b] (the caller frees them), sizes to h_hw, intrinsics to h_K */
static int load_frames(const char* path, int B, uint8_t** d_imgs, int* h_hw, double* h_K, rtm3d_frame_params* params) {
    FILE* in = fopen(path, "rb");
    uint8_t* h_img = NULL;
    int32_t n = 0, resize_to;
    int b, rc = 1;
    if (!in) { fprintf(stderr, "engine_track_frames: cannot open %s\n", path); return 1; }
    READ(&n, sizeof n, 1);
    if (n != B) { fprintf(stderr, "engine_track_frames: %s holds %d frames, the engine runs batches of %d\n", path, (int)n, B); goto done; }
    for (b = 0; b < B; ++b) {
        int32_t hw[2];
        size_t bytes;
        READ(hw, sizeof(int32_t), 2);
        if (hw[0] < 1 || hw[1] < 1 || hw[0] > 16384 || hw[1] > 16384) {
            fprintf(stderr, "engine_track_frames: %s: frame %d has size %d x %d\n", path, b, (int)hw[0], (int)hw[1]);
            goto done;
        }
        h_hw[2 * b] = hw[0]; h_hw[2 * b + 1] = hw[1];
        bytes = (size_t)hw[0] * hw[1] * 3;
        free(h_img);
        h_img = (uint8_t*)malloc(bytes);
        if (!h_img) { fprintf(stderr, "engine_track_frames: out of host memory\n"); goto done; }
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

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s ENGINE IDS.i32 FRAMES.bin [FRAMES.bin ...] [optimal]\n", argv[0]);
        return 2;
    }
    int rc = 1, b, f, n_files = argc - 3, B, params_set = 0, tracked = 0, optimal = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params fparams;
    rtm3d_track_params tparams;
    int* h_hw = NULL;
    uint8_t** d_imgs = NULL;
    float* d_rec = NULL;
    double *h_K = NULL, *d_K = NULL, *d_state = NULL;
    int32_t *d_ids = NULL, *h_ids = NULL;
    void *d_ws = NULL, *d_tws = NULL;
    hipStream_t stream = NULL;
    size_t n_slots, i;
    FILE* out = NULL;

    if (n_files > 1 && strcmp(argv[argc - 1], "optimal") == 0) { optimal = 1; --n_files; }
    if (rtm3d_engine_load(argv[1], 0, &ctx, &info) != 0) {
        fprintf(stderr, "engine_track_frames: %s\n", rtm3d_last_error());
        return 1;
    }
    B = info.B;
    n_slots = (size_t)B * info.topk;
    h_hw = (int*)malloc((size_t)B * 2 * sizeof(int));
    d_imgs = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)B * 9 * sizeof(double));
    h_ids = (int32_t*)malloc(n_slots * sizeof(int32_t));
    if (!h_hw || !d_imgs || !h_K || !h_ids) { fprintf(stderr, "engine_track_frames: out of host memory\n"); goto done; }
    out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "engine_track_frames: cannot write %s\n", argv[2]); goto done; }

    RT_OK(rtm3d_track_default_params(&tparams));
    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_ids, n_slots * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_state, rtm3d_tracks_state_bytes(B, TRACK_SLOTS)));
    HIP_OK(hipMalloc(&d_tws, rtm3d_tracks_workspace_bytes(B, info.topk, TRACK_SLOTS)));
    HIP_OK(hipMemsetAsync(d_state, 0, rtm3d_tracks_state_bytes(B, TRACK_SLOTS), stream));      /* all streams empty */
    for (f = 0; f < n_files; ++f) {
        if (load_frames(argv[3 + f], B, d_imgs, h_hw, h_K, &fparams) != 0) goto done;
        if (!params_set) {
            RT_OK(rtm3d_engine_set_frame_params(ctx, &fparams));
            HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
            params_set = 1;
        }
        HIP_OK(hipMemcpyAsync(d_K, h_K, (size_t)B * 9 * sizeof(double), hipMemcpyHostToDevice, stream));
        RT_OK(rtm3d_engine_detect_frames(ctx, stream, (const uint8_t* const*)d_imgs, h_hw, d_K, d_rec, NULL, d_ws));
        if (optimal)
            RT_OK(rtm3d_tracks_update_assign(stream, B, info.topk, TRACK_SLOTS, d_rec, 1.0, NULL, &tparams, RTM3D_TRACK_ASSIGN_OPTIMAL, d_state,
                                             d_ids, d_tws));
        else
            RT_OK(rtm3d_tracks_update(stream, B, info.topk, TRACK_SLOTS, d_rec, 1.0, NULL, &tparams, d_state, d_ids, d_tws));
        HIP_OK(hipMemcpyAsync(h_ids, d_ids, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));                        /* the ids of this frame are wanted on the host */
        if (fwrite(h_ids, sizeof(int32_t), n_slots, out) != n_slots) { fprintf(stderr, "engine_track_frames: cannot write %s\n", argv[2]); goto done; }
        for (i = 0, tracked = 0; i < n_slots; ++i) tracked += h_ids[i] != 0;
        printf("engine_track_frames: %s: %d tracked boxes in %d streams\n", argv[3 + f], tracked, B);
        for (b = 0; b < B; ++b) { (void)hipFree(d_imgs[b]); d_imgs[b] = NULL; }
    }
    rc = 0;
done:
    if (out && fclose(out) != 0) rc = 1;
    if (d_tws) (void)hipFree(d_tws);
    if (d_ws) (void)hipFree(d_ws);
    if (d_state) (void)hipFree(d_state);
    if (d_ids) (void)hipFree(d_ids);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_imgs) for (b = 0; b < B; ++b) if (d_imgs[b]) (void)hipFree(d_imgs[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(d_imgs); free(h_hw); free(h_K); free(h_ids);
    return rc;
}
