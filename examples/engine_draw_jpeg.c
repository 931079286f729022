/* engine_draw_jpeg.c - engine_draw_frames.c with the painted frames and the bird's-eye panels leaving as .jpg files instead of
 * PPM, from plain C (no Python, no torch, no image library): one rtm3d_frames_jpeg_encode call per kind of picture.
 *
 *   engine_draw_jpeg ENGINE FRAMES.bin FRAME PANEL [DEVICE]
 *
 * ENGINE      an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * FRAMES.bin  the input file of engine_detect_frames.c: int32 B; per frame int32 h, w and h * w * 3 bytes (uint8 HWC);
 *             B x 9 float64 camera intrinsics; float32 mean[3], std[3]; int32 resize_to
 * FRAME       output prefix: frame b with every detection painted goes to FRAME<b>.jpg (quality 90, 4:2:0; the input's bytes
 *             are taken as R G B)
 * PANEL       output prefix: the 400 x 400 bird's-eye panel of frame b at 0.2 m per pixel goes to PANEL<b>.jpg
 *
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_draw_jpeg: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_draw_jpeg: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)
#define READ(ptr, size, count) do { if (fread((ptr), (size), (count), in) != (size_t)(count)) { \
    fprintf(stderr, "engine_draw_jpeg: %s is truncated\n", argv[2]); goto done; } } while (0)
#define BEV_SIDE 400

#define QUALITY 90

static int write_file(const char* prefix, int b, const uint8_t* src, size_t bytes) {
    char path[1024];
    FILE* f;
    if (snprintf(path, sizeof path, "%s%d.jpg", prefix, b) >= (int)sizeof path) { fprintf(stderr, "engine_draw_jpeg: %s is too long\n", prefix); return 1; }
    f = fopen(path, "wb");
    if (!f || fwrite(src, 1, bytes, f) != bytes) {
        fprintf(stderr, "engine_draw_jpeg: cannot write %s\n", path);
        if (f) fclose(f);
        return 1;
    }
    return fclose(f) != 0;
}

/* B pictures on the device -> <prefix><b>.jpg: the workspace and the outputs are sized by the library, the staging is pinned */
static int encode_to_files(hipStream_t stream, int B, const uint8_t* const* d_src, const int* h_hw, const char* prefix) {
    uint16_t q_luma[64], q_chroma[64];
    size_t ws = 0, *cap = NULL, *len = NULL;
    int16_t *d_coef = NULL, *h_stage = NULL;
    uint8_t** out = NULL;
    int b, rc = 1;
    RT_OK(rtm3d_jpeg_quality_tables(QUALITY, q_luma, q_chroma));
    RT_OK(rtm3d_jpeg_encode_workspace_bytes(B, h_hw, RTM3D_JPEG_420, &ws));
    HIP_OK(hipMalloc((void**)&d_coef, ws));
    HIP_OK(hipHostMalloc((void**)&h_stage, ws, hipHostMallocDefault));
    cap = (size_t*)calloc((size_t)B, sizeof(size_t));
    len = (size_t*)calloc((size_t)B, sizeof(size_t));
    out = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    if (!cap || !len || !out) { fprintf(stderr, "engine_draw_jpeg: out of host memory\n"); goto done; }
    for (b = 0; b < B; ++b) {
        RT_OK(rtm3d_jpeg_encode_bound(h_hw[2 * b], h_hw[2 * b + 1], RTM3D_JPEG_420, 0, &cap[b]));
        out[b] = (uint8_t*)malloc(cap[b]);
        if (!out[b]) { fprintf(stderr, "engine_draw_jpeg: out of host memory\n"); goto done; }
    }
    RT_OK(rtm3d_frames_jpeg_encode(stream, B, d_src, h_hw, RTM3D_JPEG_420, q_luma, q_chroma, 0, 0, d_coef, h_stage, ws, out, cap, len, 0));
    for (b = 0; b < B; ++b)
        if (write_file(prefix, b, out[b], len[b])) goto done;
    rc = 0;
done:
    if (out) for (b = 0; b < B; ++b) free(out[b]);
    free(out); free(cap); free(len);
    if (h_stage) (void)hipHostFree(h_stage);
    if (d_coef) (void)hipFree(d_coef);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s ENGINE FRAMES.bin FRAME PANEL [DEVICE]\n", argv[0]);
        return 2;
    }
    int device = argc > 5 ? atoi(argv[5]) : 0, rc = 1;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params params;
    rtm3d_draw_params draw;
    FILE* in = NULL;
    int32_t B = 0;
    int *h_hw = NULL, b, found = 0;
    int* h_bev_hw = NULL;
    uint8_t **d_imgs = NULL, **d_panels = NULL, *h_img = NULL, *d_bev = NULL;
    float *h_rec = NULL, *d_rec = NULL;
    double *h_K = NULL, *d_K = NULL;
    void* d_ws = NULL;
    hipStream_t stream = NULL;
    size_t n_slots, i, bev_bytes = (size_t)BEV_SIDE * BEV_SIDE * 3;

    if (rtm3d_engine_load(argv[1], device, &ctx, &info) != 0) {
        fprintf(stderr, "engine_draw_jpeg: %s\n", rtm3d_last_error());
        return 1;
    }
    n_slots = (size_t)info.B * info.topk;
    in = fopen(argv[2], "rb");
    if (!in) { fprintf(stderr, "engine_draw_jpeg: cannot open %s\n", argv[2]); goto done; }
    READ(&B, sizeof B, 1);
    if (B != info.B) { fprintf(stderr, "engine_draw_jpeg: %s holds %d frames, the engine runs batches of %d\n", argv[2], (int)B, info.B); goto done; }
    h_hw = (int*)malloc((size_t)B * 2 * sizeof(int));
    d_imgs = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)B * 9 * sizeof(double));
    h_rec = (float*)malloc(n_slots * 32 * sizeof(float));
    if (!h_hw || !d_imgs || !h_K || !h_rec) { fprintf(stderr, "engine_draw_jpeg: out of host memory\n"); goto done; }
    for (b = 0; b < B; ++b) {
        int32_t hw[2];
        size_t bytes;
        READ(hw, sizeof(int32_t), 2);
        if (hw[0] < 1 || hw[1] < 1 || hw[0] > 8192 || hw[1] > 8192) {
            fprintf(stderr, "engine_draw_jpeg: frame %d has size %d x %d\n", b, (int)hw[0], (int)hw[1]);
            goto done;
        }
        h_hw[2 * b] = hw[0]; h_hw[2 * b + 1] = hw[1];
        bytes = (size_t)hw[0] * hw[1] * 3;
        free(h_img);
        h_img = (uint8_t*)malloc(bytes);
        if (!h_img) { fprintf(stderr, "engine_draw_jpeg: out of host memory\n"); goto done; }
        READ(h_img, 1, bytes);
        HIP_OK(hipMalloc((void**)&d_imgs[b], bytes));
        HIP_OK(hipMemcpy(d_imgs[b], h_img, bytes, hipMemcpyHostToDevice));
    }
    READ(h_K, sizeof(double), (size_t)B * 9);
    READ(params.mean, sizeof(float), 3);
    READ(params.std, sizeof(float), 3);
    {
        int32_t resize_to;
        READ(&resize_to, sizeof resize_to, 1);
        params.resize_to = resize_to;
    }
    if (fgetc(in) != EOF) { fprintf(stderr, "engine_draw_jpeg: %s holds more than one batch\n", argv[2]); goto done; }

    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_bev, (size_t)B * bev_bytes));
    HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
    HIP_OK(hipMemcpy(d_K, h_K, (size_t)B * 9 * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemsetAsync(d_bev, 0, (size_t)B * bev_bytes, stream));          /* the panels are the caller's: black here */
    RT_OK(rtm3d_engine_set_frame_params(ctx, &params));
    RT_OK(rtm3d_engine_detect_frames(ctx, stream, (const uint8_t* const*)d_imgs, h_hw, d_K, d_rec, NULL, d_ws));
    /* the one new call: every layer, the regressed vertices as the wireframe, the kept boxes in the panels */
    RT_OK(rtm3d_draw_default_params(&draw));
    draw.layers |= RTM3D_DRAW_BEV;
    draw.thickness = 2;
    draw.bev_h = BEV_SIDE; draw.bev_w = BEV_SIDE; draw.bev_m_per_px = 0.2;
    RT_OK(rtm3d_records_draw(stream, B, info.topk, d_rec, (uint8_t* const*)d_imgs, h_hw, d_K, &draw, d_bev));
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(h_rec, d_rec, n_slots * 32 * sizeof(float), hipMemcpyDeviceToHost));
    for (i = 0; i < n_slots; ++i) found += h_rec[i * 32 + 31] >= 1.0f;
    /* the painted frames and the panels leave as JPEG streams */
    d_panels = (uint8_t**)calloc((size_t)B, sizeof(uint8_t*));
    h_bev_hw = (int*)malloc((size_t)B * 2 * sizeof(int));
    if (!d_panels || !h_bev_hw) { fprintf(stderr, "engine_draw_jpeg: out of host memory\n"); goto done; }
    for (b = 0; b < B; ++b) { d_panels[b] = d_bev + (size_t)b * bev_bytes; h_bev_hw[2 * b] = BEV_SIDE; h_bev_hw[2 * b + 1] = BEV_SIDE; }
    if (encode_to_files(stream, B, (const uint8_t* const*)d_imgs, h_hw, argv[3])) goto done;
    if (encode_to_files(stream, B, (const uint8_t* const*)d_panels, h_bev_hw, argv[4])) goto done;
    printf("engine_draw_jpeg: %s %d frames on a %dx%d canvas, %d detections painted, %d + %d .jpg files, frame 0 %dx%d\n", info.backbone, info.B, info.H,
           info.W, found, (int)B, (int)B, h_hw[0], h_hw[1]);
    rc = 0;
done:
    if (in) fclose(in);
    if (d_ws) (void)hipFree(d_ws);
    if (d_bev) (void)hipFree(d_bev);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_imgs) for (b = 0; b < B; ++b) if (d_imgs[b]) (void)hipFree(d_imgs[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(h_img); free(d_panels); free(h_bev_hw); free(d_imgs); free(h_hw); free(h_K); free(h_rec);
    return rc;
}
