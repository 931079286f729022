/* engine_rig_frames.c - the frames of the C cameras of one vehicle in, one set of tracked 3D boxes in the rig frame out, from
 * plain C (no Python, no torch).
 *
 *   engine_rig_frames ENGINE EXTRINSICS.f64 OUT.bin FRAMES.bin [FRAMES.bin ...]
 *
 * ENGINE          an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine); its batch B is the number of cameras
 * EXTRINSICS.f64  B x 12 raw float64: per camera the row-major 3 x 4 [R | t], camera coordinates -> rig frame
 * FRAMES.bin      one per time step, in order, each in the format of engine_detect_frames.c: int32 B; per frame int32 h, w and
 *                 h * w * 3 bytes; B x 9 float64 camera intrinsics; float32 mean[3], std[3]; int32 resize_to.  Frame c of every
 *                 file is the next frame of camera c.
 * OUT.bin         output, per file: int32 clusters written, clusters dropped; cap x 7 float64 fused boxes h w l X Y Z ry (zeros in
 *                 empty slots); cap int32 rig ids (+id confirmed track, -id tentative, 0 none); B x topk int32 the same ids per
 *                 camera record slot.  cap = min(256, B * topk).
 *
 * Per file, on one stream and without a synchronisation in between: rtm3d_engine_detect_frames, rtm3d_rig_fuse with the default
 * parameters (rtm3d_rig_default_params), rtm3d_tracks_update on the fused records (one stream, 128 track slots, default
 * parameters, dt = 1, no ego motion), rtm3d_rig_scatter_ids.  The fused boxes are also printed, one per line.
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define TRACK_SLOTS 128
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_rig_frames: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_rig_frames: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)
#define READ(ptr, size, count) do { if (fread((ptr), (size), (count), in) != (size_t)(count)) { \
    fprintf(stderr, "engine_rig_frames: %s is truncated\n", path); goto done; } } while (0)
#define WRITE(ptr, size, count) do { if (fwrite((ptr), (size), (count), out) != (size_t)(count)) { \
    fprintf(stderr, "engine_rig_frames: cannot write %s\n", argv[3]); goto done; } } while (0)

/* one FRAMES.bin: the frames go to fresh device buffers d_imgs[b] (the caller frees them), sizes to h_hw, intrinsics to h_K */
static int load_frames(const char* path, int B, uint8_t** d_imgs, int* h_hw, double* h_K, rtm3d_frame_params* params) {
    FILE* in = fopen(path, "rb");
    uint8_t* h_img = NULL;
    int32_t n = 0, resize_to;
    int b, rc = 1;
    if (!in) { fprintf(stderr, "engine_rig_frames: cannot open %s\n", path); return 1; }
    READ(&n, sizeof n, 1);
    if (n != B) { fprintf(stderr, "engine_rig_frames: %s holds %d frames, the engine runs batches of %d\n", path, (int)n, B); goto done; }
    for (b = 0; b < B; ++b) {
        int32_t hw[2];
        size_t bytes;
        READ(hw, sizeof(int32_t), 2);
        if (hw[0] < 1 || hw[1] < 1 || hw[0] > 16384 || hw[1] > 16384) {
            fprintf(stderr, "engine_rig_frames: %s: frame %d has size %d x %d\n", path, b, (int)hw[0], (int)hw[1]);
            goto done;
        }
        h_hw[2 * b] = hw[0]; h_hw[2 * b + 1] = hw[1];
        bytes = (size_t)hw[0] * hw[1] * 3;
        free(h_img);
        h_img = (uint8_t*)malloc(bytes);
        if (!h_img) { fprintf(stderr, "engine_rig_frames: out of host memory\n"); goto done; }
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
    if (argc < 5) {
        fprintf(stderr, "usage: %s ENGINE EXTRINSICS.f64 OUT.bin FRAMES.bin [FRAMES.bin ...]\n", argv[0]);
        return 2;
    }
    int rc = 1, b, f, s, n_files = argc - 4, B, cap, params_set = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params fparams;
    rtm3d_track_params tparams;
    rtm3d_rig_params rparams;
    int* h_hw = NULL;
    uint8_t** d_imgs = NULL;
    float *d_rec = NULL, *d_fused = NULL;
    double *h_K = NULL, *d_K = NULL, *h_ext = NULL, *d_ext = NULL, *d_state = NULL, *d_box = NULL, *h_box = NULL;
    int32_t *d_info = NULL, *d_map = NULL, *d_n = NULL, *d_ids_rig = NULL, *d_ids_cam = NULL, *h_ids_rig = NULL, *h_ids_cam = NULL;
    int32_t h_n[2];
    void *d_ws = NULL, *d_tws = NULL, *d_rws = NULL;
    hipStream_t stream = NULL;
    size_t n_slots;
    FILE *out = NULL, *in = NULL;
    const char* path = argv[2];

    if (rtm3d_engine_load(argv[1], 0, &ctx, &info) != 0) {
        fprintf(stderr, "engine_rig_frames: %s\n", rtm3d_last_error());
        return 1;
    }
    B = info.B;
    n_slots = (size_t)B * info.topk;
    cap = n_slots < 256 ? (int)n_slots : 256;
    if (rtm3d_rig_workspace_bytes(1, B, info.topk) == 0) {
        fprintf(stderr, "engine_rig_frames: a rig of %d cameras with %d record slots each is more than rtm3d_rig_fuse takes\n", B, info.topk);
        goto done;
    }
    h_hw = (int*)malloc((size_t)B * 2 * sizeof(int));
    d_imgs = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)B * 9 * sizeof(double));
    h_ext = (double*)malloc((size_t)B * 12 * sizeof(double));
    h_box = (double*)malloc((size_t)cap * 7 * sizeof(double));
    h_ids_rig = (int32_t*)malloc((size_t)cap * sizeof(int32_t));
    h_ids_cam = (int32_t*)malloc(n_slots * sizeof(int32_t));
    if (!h_hw || !d_imgs || !h_K || !h_ext || !h_box || !h_ids_rig || !h_ids_cam) { fprintf(stderr, "engine_rig_frames: out of host memory\n"); goto done; }
    in = fopen(path, "rb");
    if (!in) { fprintf(stderr, "engine_rig_frames: cannot open %s\n", path); goto done; }
    READ(h_ext, sizeof(double), (size_t)B * 12);
    out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "engine_rig_frames: cannot write %s\n", argv[3]); goto done; }

    RT_OK(rtm3d_track_default_params(&tparams));
    RT_OK(rtm3d_rig_default_params(&rparams));
    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_ext, (size_t)B * 12 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_fused, (size_t)cap * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_box, (size_t)cap * 7 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_info, (size_t)cap * 4 * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_map, n_slots * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_n, 2 * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_ids_rig, (size_t)cap * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&d_ids_cam, n_slots * sizeof(int32_t)));
    HIP_OK(hipMalloc(&d_rws, rtm3d_rig_workspace_bytes(1, B, info.topk)));
    HIP_OK(hipMalloc((void**)&d_state, rtm3d_tracks_state_bytes(1, TRACK_SLOTS)));
    HIP_OK(hipMalloc(&d_tws, rtm3d_tracks_workspace_bytes(1, cap, TRACK_SLOTS)));
    HIP_OK(hipMemsetAsync(d_state, 0, rtm3d_tracks_state_bytes(1, TRACK_SLOTS), stream));      /* the rig's one stream, empty */
    HIP_OK(hipMemcpyAsync(d_ext, h_ext, (size_t)B * 12 * sizeof(double), hipMemcpyHostToDevice, stream));
    for (f = 0; f < n_files; ++f) {
        if (load_frames(argv[4 + f], B, d_imgs, h_hw, h_K, &fparams) != 0) goto done;
        if (!params_set) {
            RT_OK(rtm3d_engine_set_frame_params(ctx, &fparams));
            HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
            params_set = 1;
        }
        HIP_OK(hipMemcpyAsync(d_K, h_K, (size_t)B * 9 * sizeof(double), hipMemcpyHostToDevice, stream));
        RT_OK(rtm3d_engine_detect_frames(ctx, stream, (const uint8_t* const*)d_imgs, h_hw, d_K, d_rec, NULL, d_ws));
        RT_OK(rtm3d_rig_fuse(stream, 1, B, info.topk, cap, d_rec, d_ext, &rparams, d_fused, d_box, d_info, d_map, d_n, d_rws));
        RT_OK(rtm3d_tracks_update(stream, 1, cap, TRACK_SLOTS, d_fused, 1.0, NULL, &tparams, d_state, d_ids_rig, d_tws));
        RT_OK(rtm3d_rig_scatter_ids(stream, 1, B, info.topk, cap, d_map, d_ids_rig, d_ids_cam));
        HIP_OK(hipMemcpyAsync(h_n, d_n, sizeof h_n, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(h_box, d_box, (size_t)cap * 7 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(h_ids_rig, d_ids_rig, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(h_ids_cam, d_ids_cam, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));                        /* the boxes and ids of this step are wanted on the host */
        WRITE(h_n, sizeof(int32_t), 2);
        WRITE(h_box, sizeof(double), (size_t)cap * 7);
        WRITE(h_ids_rig, sizeof(int32_t), (size_t)cap);
        WRITE(h_ids_cam, sizeof(int32_t), n_slots);
        printf("engine_rig_frames: %s: %d fused boxes from %d cameras, %d dropped\n", argv[4 + f], (int)h_n[0], B, (int)h_n[1]);
        for (s = 0; s < h_n[0]; ++s)
            printf("  id %d  h %.4f w %.4f l %.4f  X %.4f Y %.4f Z %.4f  ry %.4f\n", (int)h_ids_rig[s], h_box[7 * s], h_box[7 * s + 1],
                   h_box[7 * s + 2], h_box[7 * s + 3], h_box[7 * s + 4], h_box[7 * s + 5], h_box[7 * s + 6]);
        for (b = 0; b < B; ++b) { (void)hipFree(d_imgs[b]); d_imgs[b] = NULL; }
    }
    rc = 0;
done:
    if (in) fclose(in);
    if (out && fclose(out) != 0) rc = 1;
    if (d_tws) (void)hipFree(d_tws);
    if (d_rws) (void)hipFree(d_rws);
    if (d_ws) (void)hipFree(d_ws);
    if (d_state) (void)hipFree(d_state);
    if (d_ids_cam) (void)hipFree(d_ids_cam);
    if (d_ids_rig) (void)hipFree(d_ids_rig);
    if (d_n) (void)hipFree(d_n);
    if (d_map) (void)hipFree(d_map);
    if (d_info) (void)hipFree(d_info);
    if (d_box) (void)hipFree(d_box);
    if (d_fused) (void)hipFree(d_fused);
    if (d_rec) (void)hipFree(d_rec);
    if (d_ext) (void)hipFree(d_ext);
    if (d_K) (void)hipFree(d_K);
    if (d_imgs) for (b = 0; b < B; ++b) if (d_imgs[b]) (void)hipFree(d_imgs[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(d_imgs); free(h_hw); free(h_K); free(h_ext); free(h_box); free(h_ids_rig); free(h_ids_cam);
    return rc;
}
