/* engine_detect_jpeg.c - JPEG files in, KITTI rows out, from plain C (no Python, no torch, no image library).
 *
 *   engine_detect_jpeg ENGINE PARAMS.bin FRAME.jpg [FRAME.jpg ...] [-d DEVICE]
 *
 * ENGINE       an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * PARAMS.bin   little-endian: B x 9 float64 camera intrinsics (row-major 3 x 3 per frame, the camera's own); float32 mean[3],
 *              std[3]; int32 resize_to (0: frames are fed at their own size); int32 dst_order (0 R G B, 1 B G R: the order the
 *              checkpoint was trained on)
 * FRAME.jpg    one per frame of the engine's batch: a baseline JPEG (grey, 4:4:4, 4:2:2 or 4:2:0), of any size that fits the
 *              engine's canvas after Resize
 *
 * rtm3d_jpeg_info tells the size of every frame, rtm3d_jpeg_workspace_bytes the size of the pinned staging buffer and of the
 * device coefficient buffer; rtm3d_engine_detect_frames_jpeg entropy-decodes on the host, copies, runs the inverse DCT and the
 * colour conversion on the device and detects, in one stream-ordered step.  Prints one line per detection: frame, slot, class,
 * score and the 2D box x1 y1 x2 y2 in the pixels of the frame (%.9g: the text identifies the floats) and, for a box the 3D
 * solver kept, " |" and the 16 numbers of its KITTI row (%.17g).
 *
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so, libamdhip64 and libm only).                            */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_detect_jpeg: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_detect_jpeg: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)

int main(int argc, char** argv) {
    int device = 0, rc = 1, b, k, nfiles, kept = 0, found = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params params;
    rtm3d_jpeg_stream_info ji;
    int32_t tail[2];
    uint8_t **h_data = NULL, **d_packed = NULL;
    size_t *h_bytes = NULL, *packed_bytes = NULL, n_slots, i, coef_bytes = 0;
    int16_t *h_stage = NULL, *d_coef = NULL;
    double *h_K = NULL, *d_K = NULL, *h_kitti = NULL, *d_kitti = NULL;
    float *h_rec = NULL, *d_rec = NULL;
    void* d_ws = NULL;
    hipStream_t stream = NULL;
    FILE* in = NULL;

    memset(&info, 0, sizeof info);
    if (argc >= 3 && strcmp(argv[argc - 2], "-d") == 0) { device = atoi(argv[argc - 1]); argc -= 2; }
    if (argc < 4) {
        fprintf(stderr, "usage: %s ENGINE PARAMS.bin FRAME.jpg [FRAME.jpg ...] [-d DEVICE]\n", argv[0]);
        return 2;
    }
    nfiles = argc - 3;
    if (rtm3d_engine_load(argv[1], device, &ctx, &info) != 0) {
        fprintf(stderr, "engine_detect_jpeg: %s\n", rtm3d_last_error());
        return 1;
    }
    if (nfiles != info.B) { fprintf(stderr, "engine_detect_jpeg: %d frame files, the engine runs batches of %d\n", nfiles, info.B); goto done; }
    n_slots = (size_t)info.B * info.topk;
    h_data = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    d_packed = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    h_bytes = (size_t*)calloc((size_t)info.B, sizeof(size_t));
    packed_bytes = (size_t*)calloc((size_t)info.B, sizeof(size_t));
    h_K = (double*)malloc((size_t)info.B * 9 * sizeof(double));
    h_kitti = (double*)malloc(n_slots * 16 * sizeof(double));
    h_rec = (float*)malloc(n_slots * 32 * sizeof(float));
    if (!h_data || !d_packed || !h_bytes || !packed_bytes || !h_K || !h_kitti || !h_rec) { fprintf(stderr, "engine_detect_jpeg: out of host memory\n"); goto done; }

    in = fopen(argv[2], "rb");
    if (!in || fread(h_K, sizeof(double), (size_t)info.B * 9, in) != (size_t)info.B * 9 || fread(params.mean, sizeof(float), 3, in) != 3 ||
        fread(params.std, sizeof(float), 3, in) != 3 || fread(tail, sizeof(int32_t), 2, in) != 2) {
        fprintf(stderr, "engine_detect_jpeg: cannot read %s\n", argv[2]);
        goto done;
    }
    fclose(in); in = NULL;
    params.resize_to = tail[0];

    for (b = 0; b < info.B; ++b) {
        long len;
        in = fopen(argv[3 + b], "rb");
        if (!in || fseek(in, 0, SEEK_END) != 0 || (len = ftell(in)) <= 0 || fseek(in, 0, SEEK_SET) != 0) {
            fprintf(stderr, "engine_detect_jpeg: cannot read %s\n", argv[3 + b]);
            goto done;
        }
        h_data[b] = (uint8_t*)malloc((size_t)len);
        if (!h_data[b] || fread(h_data[b], 1, (size_t)len, in) != (size_t)len) { fprintf(stderr, "engine_detect_jpeg: cannot read %s\n", argv[3 + b]); goto done; }
        fclose(in); in = NULL;
        h_bytes[b] = (size_t)len;
        if (rtm3d_jpeg_info(h_data[b], h_bytes[b], &ji) != 0) { fprintf(stderr, "engine_detect_jpeg: %s: %s\n", argv[3 + b], rtm3d_last_error()); goto done; }
        packed_bytes[b] = (size_t)ji.h * ji.w * 3;
        HIP_OK(hipMalloc((void**)&d_packed[b], packed_bytes[b]));
    }
    RT_OK(rtm3d_jpeg_workspace_bytes(info.B, (const uint8_t* const*)h_data, h_bytes, &coef_bytes));
    HIP_OK(hipHostMalloc((void**)&h_stage, coef_bytes, hipHostMallocDefault));          /* pinned: the copy is asynchronous */
    HIP_OK(hipMalloc((void**)&d_coef, coef_bytes));

    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)info.B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_kitti, n_slots * 16 * sizeof(double)));
    HIP_OK(hipMemcpy(d_K, h_K, (size_t)info.B * 9 * sizeof(double), hipMemcpyHostToDevice));
    RT_OK(rtm3d_engine_set_frame_params(ctx, &params));
    HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
    RT_OK(rtm3d_engine_detect_frames_jpeg(ctx, stream, (const uint8_t* const*)h_data, h_bytes, h_stage, d_coef, coef_bytes,
                                          (uint8_t* const*)d_packed, packed_bytes, tail[1], 0, d_K, d_rec, d_kitti, d_ws));
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(h_kitti, d_kitti, n_slots * 16 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_rec, d_rec, n_slots * 32 * sizeof(float), hipMemcpyDeviceToHost));
    printf("engine_detect_jpeg: %s %d JPEG frames (%zu coefficient bytes) on a %dx%d canvas\n", info.backbone, info.B, coef_bytes, info.H, info.W);
    for (i = 0; i < n_slots; ++i) {
        const float* r = h_rec + i * 32;
        if (r[31] < 1.0f) continue;
        ++found;
        printf("%d %d %d %.9g %.9g %.9g %.9g %.9g", (int)(i / (size_t)info.topk), (int)(i % (size_t)info.topk), (int)r[0], r[1], r[20], r[21],
               r[22], r[23]);
        if (h_kitti[i * 16 + 14] == 2.0) {
            ++kept;
            printf(" |");
            for (k = 0; k < 16; ++k) printf(" %.17g", h_kitti[i * 16 + k]);
        }
        printf("\n");
    }
    printf("engine_detect_jpeg: %d detections, %d KITTI rows\n", found, kept);
    rc = 0;
done:
    if (in) fclose(in);
    if (d_ws) (void)hipFree(d_ws);
    if (d_kitti) (void)hipFree(d_kitti);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_coef) (void)hipFree(d_coef);
    if (h_stage) (void)hipHostFree(h_stage);
    if (d_packed) for (b = 0; b < info.B; ++b) if (d_packed[b]) (void)hipFree(d_packed[b]);
    if (h_data) for (b = 0; b < info.B; ++b) free(h_data[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(h_data); free(d_packed); free(h_bytes); free(packed_bytes); free(h_K); free(h_kitti); free(h_rec);
    return rc;
}
