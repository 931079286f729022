/* engine_detect.c - run one detect step of an engine file from plain C (no Python, no torch).
 *
 *   engine_detect ENGINE IMAGES.f32 K.f64 RECORDS.f32 [DEVICE]
 *
 * ENGINE      an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * IMAGES.f32  the normalised batch: B x 3 x H x W raw little-endian float32 (NCHW), B, H, W of the engine
 * K.f64       B x 9 raw float64 camera intrinsics (row-major 3 x 3 per image)
 * RECORDS.f32 output: B x topk x 32 raw float32 detection records (layout of rtm3d_pack_records in rtm3d_hip.h)
 *
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

static int read_file(const char* path, void* dst, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "engine_detect: cannot open %s\n", path); return 1; }
    size_t got = fread(dst, 1, bytes, f);
    int extra = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || extra) { fprintf(stderr, "engine_detect: %s must hold exactly %zu bytes\n", path, bytes); return 1; }
    return 0;
}

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_detect: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_detect: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s ENGINE IMAGES.f32 K.f64 RECORDS.f32 [DEVICE]\n", argv[0]);
        return 2;
    }
    int device = argc > 5 ? atoi(argv[5]) : 0, rc = 1;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    float *h_in = NULL, *h_rec = NULL, *d_in = NULL, *d_rec = NULL;
    double *h_K = NULL, *d_K = NULL;
    void* d_ws = NULL;
    hipStream_t stream = NULL;
    size_t n_in, n_rec;
    int kept = 0, found = 0;

    if (rtm3d_engine_load(argv[1], device, &ctx, &info) != 0) {
        fprintf(stderr, "engine_detect: %s\n", rtm3d_last_error());
        return 1;
    }
    n_in = (size_t)info.B * 3 * info.H * info.W;
    n_rec = (size_t)info.B * info.topk * 32;
    h_in = (float*)malloc(n_in * sizeof(float));
    h_K = (double*)malloc((size_t)info.B * 9 * sizeof(double));
    h_rec = (float*)malloc(n_rec * sizeof(float));
    if (!h_in || !h_K || !h_rec) { fprintf(stderr, "engine_detect: out of host memory\n"); goto done; }
    if (read_file(argv[2], h_in, n_in * sizeof(float)) || read_file(argv[3], h_K, (size_t)info.B * 9 * sizeof(double))) goto done;

    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_in, n_in * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)info.B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_rec * sizeof(float)));
    HIP_OK(hipMalloc(&d_ws, rtm3d_engine_workspace_bytes(ctx)));
    HIP_OK(hipMemcpy(d_in, h_in, n_in * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_K, h_K, (size_t)info.B * 9 * sizeof(double), hipMemcpyHostToDevice));
    RT_OK(rtm3d_engine_detect(ctx, stream, d_in, d_K, d_rec, d_ws));
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(h_rec, d_rec, n_rec * sizeof(float), hipMemcpyDeviceToHost));
    {
        FILE* f = fopen(argv[4], "wb");
        if (!f || fwrite(h_rec, sizeof(float), n_rec, f) != n_rec) {
            fprintf(stderr, "engine_detect: cannot write %s\n", argv[4]);
            if (f) fclose(f);
            goto done;
        }
        fclose(f);
    }
    for (size_t i = 0; i < n_rec; i += 32) {
        found += h_rec[i + 31] >= 1.0f;
        kept += h_rec[i + 31] >= 2.0f;
    }
    printf("engine_detect: %s %dx3x%dx%d, %d detections, %d 3D boxes kept\n", info.backbone, info.B, info.H, info.W, found, kept);
    rc = 0;
done:
    if (d_ws) (void)hipFree(d_ws);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_in) (void)hipFree(d_in);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(h_in); free(h_K); free(h_rec);
    return rc;
}
