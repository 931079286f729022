/* engine_detect_lens.c - a decoder surface of a real (distorting) lens in, KITTI rows of the rectified frame out, from plain C.
 *
 *   engine_detect_lens ENGINE PARAMS.bin W H FRAME.nv12 FX FY CX CY K1 K2 P1 P2 K3 [-d DEVICE]
 *
 * ENGINE      an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * PARAMS.bin  the file of engine_detect_nv12: B x 9 float64 intrinsics - here those of the RECTIFIED frames, row-major 3 x 3 per
 *             frame; float32 mean[3], std[3]; int32 resize_to, matrix (0 BT.601, 1 BT.709), range (0 limited, 1 full),
 *             dst_order (0 R G B, 1 B G R)
 * W H         the size of the lens's frames; the rectified frames have the same size
 * FRAME.nv12  W x H bytes of Y, then (W + 1) / 2 x (H + 1) / 2 pairs Cb Cr, no padding; every frame of the batch is this file
 * FX .. K3    the lens: its own intrinsics and the five coefficients of the Brown model
 *
 * rtm3d_lens_map_build makes one map (frame 0's rectified intrinsics, no rotation) that all frames share; then
 * rtm3d_engine_detect_frames_lens converts the surfaces, resamples them through the map and detects, in one stream-ordered
 * step.  Prints one line per detection - frame, slot, class, score and the 2D box x1 y1 x2 y2 in the pixels of the RECTIFIED
 * frame (%.9g) and, for a box the 3D solver kept, " |" and the 16 numbers of its KITTI row (%.17g) - and a checksum (the sum of
 * the bytes) of rectified frame 0.
 *
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so and libamdhip64 only).                                 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_detect_lens: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_detect_lens: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)

int main(int argc, char** argv) {
    int device = 0, rc = 1, b, k, w, h, cw, ch, pitch, kept = 0, found = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params params;
    rtm3d_frame_src* src = NULL;
    rtm3d_lens_model model;
    rtm3d_lens_rect rect;
    rtm3d_lens_map* maps = NULL;
    const uint8_t fill[3] = {0, 0, 0};
    int32_t tail[4];
    int32_t* d_map = NULL;
    uint8_t *d_surface = NULL, **d_packed = NULL, **d_rect = NULL, *h_file = NULL, *h_rect = NULL;
    double *h_K = NULL, *d_K = NULL, *h_kitti = NULL, *d_kitti = NULL;
    float *h_rec = NULL, *d_rec = NULL;
    void* d_ws = NULL;
    hipStream_t stream = NULL;
    FILE* in = NULL;
    size_t n_slots, i, file_bytes;
    unsigned long long sum = 0;

    memset(&info, 0, sizeof info);
    if (argc >= 3 && strcmp(argv[argc - 2], "-d") == 0) { device = atoi(argv[argc - 1]); argc -= 2; }
    if (argc != 15) {
        fprintf(stderr, "usage: %s ENGINE PARAMS.bin W H FRAME.nv12 FX FY CX CY K1 K2 P1 P2 K3 [-d DEVICE]\n", argv[0]);
        return 2;
    }
    w = atoi(argv[3]); h = atoi(argv[4]);
    if (w < 1 || h < 1 || w > 16384 || h > 16384) { fprintf(stderr, "engine_detect_lens: a frame of %d x %d\n", w, h); return 2; }
    cw = (w + 1) / 2; ch = (h + 1) / 2;
    pitch = (w > 2 * cw ? w : 2 * cw);
    pitch = (pitch + 255) / 256 * 256;
    file_bytes = (size_t)w * h + (size_t)2 * cw * ch;
    memset(&model, 0, sizeof model);
    memset(&rect, 0, sizeof rect);
    model.kind = RTM3D_LENS_BROWN; model.h = h; model.w = w;
    model.K[0] = atof(argv[6]); model.K[4] = atof(argv[7]); model.K[2] = atof(argv[8]); model.K[5] = atof(argv[9]); model.K[8] = 1.0;
    model.dist[0] = atof(argv[10]); model.dist[1] = atof(argv[11]); model.dist[2] = atof(argv[12]); model.dist[3] = atof(argv[13]);
    model.dist[4] = atof(argv[14]);

    if (rtm3d_engine_load(argv[1], device, &ctx, &info) != 0) {
        fprintf(stderr, "engine_detect_lens: %s\n", rtm3d_last_error());
        return 1;
    }
    n_slots = (size_t)info.B * info.topk;
    src = (rtm3d_frame_src*)calloc((size_t)info.B, sizeof *src);
    maps = (rtm3d_lens_map*)calloc((size_t)info.B, sizeof *maps);
    d_packed = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    d_rect = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)info.B * 9 * sizeof(double));
    h_kitti = (double*)malloc(n_slots * 16 * sizeof(double));
    h_rec = (float*)malloc(n_slots * 32 * sizeof(float));
    h_file = (uint8_t*)malloc(file_bytes);
    h_rect = (uint8_t*)malloc((size_t)h * w * 3);
    if (!src || !maps || !d_packed || !d_rect || !h_K || !h_kitti || !h_rec || !h_file || !h_rect) {
        fprintf(stderr, "engine_detect_lens: out of host memory\n");
        goto done;
    }

    in = fopen(argv[2], "rb");
    if (!in || fread(h_K, sizeof(double), (size_t)info.B * 9, in) != (size_t)info.B * 9 || fread(params.mean, sizeof(float), 3, in) != 3 ||
        fread(params.std, sizeof(float), 3, in) != 3 || fread(tail, sizeof(int32_t), 4, in) != 4) {
        fprintf(stderr, "engine_detect_lens: cannot read %s\n", argv[2]);
        goto done;
    }
    fclose(in); in = NULL;
    params.resize_to = tail[0];
    in = fopen(argv[5], "rb");
    if (!in || fread(h_file, 1, file_bytes, in) != file_bytes || fgetc(in) != EOF) {
        fprintf(stderr, "engine_detect_lens: %s is not a %d x %d NV12 frame of %zu bytes\n", argv[5], w, h, file_bytes);
        goto done;
    }
    fclose(in); in = NULL;

    HIP_OK(hipStreamCreate(&stream));
    /* one pitched surface, as a decoder hands it over: h luma rows, then ch chroma rows */
    HIP_OK(hipMalloc((void**)&d_surface, (size_t)pitch * (h + ch)));
    HIP_OK(hipMemcpy2D(d_surface, (size_t)pitch, h_file, (size_t)w, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy2D(d_surface + (size_t)pitch * h, (size_t)pitch, h_file + (size_t)w * h, (size_t)2 * cw, (size_t)2 * cw, (size_t)ch,
                       hipMemcpyHostToDevice));
    /* the map: the rectified camera of frame 0, no rotation, the lens's own size */
    rect.ho = h; rect.wo = w;
    memcpy(rect.K, h_K, sizeof rect.K);
    rect.R[0] = rect.R[4] = rect.R[8] = 1.0;
    HIP_OK(hipMalloc((void**)&d_map, (size_t)h * w * 2 * sizeof(int32_t)));
    RT_OK(rtm3d_lens_map_build(stream, 1, &model, &rect, (int32_t* const*)&d_map));
    for (b = 0; b < info.B; ++b) {
        HIP_OK(hipMalloc((void**)&d_packed[b], (size_t)h * w * 3));
        HIP_OK(hipMalloc((void**)&d_rect[b], (size_t)h * w * 3));
        src[b].plane[0] = d_surface;
        src[b].plane[1] = d_surface + (size_t)pitch * h;
        src[b].pitch[0] = src[b].pitch[1] = pitch;
        src[b].h = h; src[b].w = w;
        src[b].format = RTM3D_PIX_NV12; src[b].matrix = tail[1]; src[b].range = tail[2];
        maps[b].d_map = d_map; maps[b].ho = h; maps[b].wo = w;
    }
    HIP_OK(hipMalloc((void**)&d_K, (size_t)info.B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_kitti, n_slots * 16 * sizeof(double)));
    HIP_OK(hipMemcpy(d_K, h_K, (size_t)info.B * 9 * sizeof(double), hipMemcpyHostToDevice));
    RT_OK(rtm3d_engine_set_frame_params(ctx, &params));
    HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
    RT_OK(rtm3d_engine_detect_frames_lens(ctx, stream, src, (uint8_t* const*)d_packed, NULL, tail[3], maps, (uint8_t* const*)d_rect, fill,
                                          d_K, d_rec, d_kitti, d_ws));
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(h_kitti, d_kitti, n_slots * 16 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_rec, d_rec, n_slots * 32 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_rect, d_rect[0], (size_t)h * w * 3, hipMemcpyDeviceToHost));
    for (i = 0; i < (size_t)h * w * 3; ++i) sum += h_rect[i];
    printf("engine_detect_lens: %s %d NV12 frames of %dx%d (pitch %d) rectified on a %dx%d canvas\n", info.backbone, info.B, h, w, pitch,
           info.H, info.W);
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
    printf("engine_detect_lens: %d detections, %d KITTI rows, rectified frame 0 sums to %llu\n", found, kept, sum);
    rc = 0;
done:
    if (in) fclose(in);
    if (d_ws) (void)hipFree(d_ws);
    if (d_kitti) (void)hipFree(d_kitti);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_map) (void)hipFree(d_map);
    if (d_surface) (void)hipFree(d_surface);
    if (d_packed) for (b = 0; b < info.B; ++b) if (d_packed[b]) (void)hipFree(d_packed[b]);
    if (d_rect) for (b = 0; b < info.B; ++b) if (d_rect[b]) (void)hipFree(d_rect[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(src); free(maps); free(d_packed); free(d_rect); free(h_K); free(h_kitti); free(h_rec); free(h_file); free(h_rect);
    return rc;
}
