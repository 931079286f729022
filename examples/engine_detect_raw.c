/* engine_detect_raw.c - raw Bayer sensor frames in, KITTI rows out, from plain C (no Python, no torch).
 *
 *   engine_detect_raw ENGINE PARAMS.bin W H FRAME.raw10 [FRAME.raw10 ...] [-d DEVICE]
 *
 * ENGINE       an engine file written by rtm3d_amd.engine.save_engine (Model.save_engine)
 * PARAMS.bin   little-endian: B x 9 float64 camera intrinsics (row-major 3 x 3 per frame, the camera's own); float32 mean[3],
 *              std[3]; int32 resize_to (0: frames are fed at their own size); int32 pattern (RTM3D_CFA_*), method
 *              (RTM3D_DEMOSAIC_*), dst_order (0 R G B, 1 B G R: the order the checkpoint was trained on); int32 black level;
 *              float32 white-balance gains r, g, b
 * W H          the size of every frame
 * FRAME.raw10  one per frame of the engine's batch: H rows of 5 * ceil(W / 4) bytes, MIPI CSI-2 RAW10 (four samples' high
 *              bytes, then one byte with their low bit pairs), no padding
 *
 * Every file is uploaded at a row pitch rounded up to 256 bytes and described by an rtm3d_raw_src that carries the black
 * level, the gains in Q10, the identity colour matrix and an sRGB tone table built here with pow();
 * rtm3d_engine_detect_frames_raw demosaics and detects in one stream-ordered step.  Prints one line per detection: frame,
 * slot, class, score and the 2D box x1 y1 x2 y2 in the pixels of the frame (%.9g: the text identifies the floats) and, for a
 * box the 3D solver kept, " |" and the 16 numbers of its KITTI row (%.17g).
 *
 * Build: make -C rtm3d_amd/csrc example  (links librtm3d_hip.so, libamdhip64 and libm only).                            */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../include/rtm3d_hip.h"

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fprintf(stderr, "engine_detect_raw: %s: %s\n", #expr, hipGetErrorString(e_)); goto done; } } while (0)
#define RT_OK(expr) do { if ((expr) != 0) { fprintf(stderr, "engine_detect_raw: %s: %s\n", #expr, rtm3d_last_error()); goto done; } } while (0)

/* colour (0 R, 1 G, 2 B) of cells k = (y & 1) * 2 + (x & 1) of the four patterns */
static const int cell_colour[4][4] = {{0, 1, 1, 2}, {2, 1, 1, 0}, {1, 0, 2, 1}, {1, 2, 0, 1}};

int main(int argc, char** argv) {
    int device = 0, rc = 1, b, k, nfiles, w, h, row, pitch, kept = 0, found = 0;
    rtm3d_ctx* ctx = NULL;
    rtm3d_engine_info info;
    rtm3d_frame_params params;
    rtm3d_raw_src* src = NULL;
    int32_t tail[5];
    float wb[3];
    uint8_t **d_plane = NULL, **d_packed = NULL, *h_file = NULL, *d_tone = NULL, h_tone[4096];
    double *h_K = NULL, *d_K = NULL, *h_kitti = NULL, *d_kitti = NULL;
    float *h_rec = NULL, *d_rec = NULL;
    void* d_ws = NULL;
    hipStream_t stream = NULL;
    FILE* in = NULL;
    size_t n_slots, i, file_bytes;

    if (argc >= 3 && strcmp(argv[argc - 2], "-d") == 0) { device = atoi(argv[argc - 1]); argc -= 2; }
    if (argc < 6) {
        fprintf(stderr, "usage: %s ENGINE PARAMS.bin W H FRAME.raw10 [FRAME.raw10 ...] [-d DEVICE]\n", argv[0]);
        return 2;
    }
    w = atoi(argv[3]); h = atoi(argv[4]); nfiles = argc - 5;
    if (w < 2 || h < 2 || w > 16384 || h > 16384) { fprintf(stderr, "engine_detect_raw: a frame of %d x %d\n", w, h); return 2; }
    if (rtm3d_raw_src_layout(RTM3D_RAW_MIPI10, 10, h, w, &row, &k) != 0) { fprintf(stderr, "engine_detect_raw: %s\n", rtm3d_last_error()); return 1; }
    pitch = (row + 255) / 256 * 256;
    file_bytes = (size_t)row * h;

    if (rtm3d_engine_load(argv[1], device, &ctx, &info) != 0) {
        fprintf(stderr, "engine_detect_raw: %s\n", rtm3d_last_error());
        return 1;
    }
    if (nfiles != info.B) { fprintf(stderr, "engine_detect_raw: %d frame files, the engine runs batches of %d\n", nfiles, info.B); goto done; }
    n_slots = (size_t)info.B * info.topk;
    src = (rtm3d_raw_src*)calloc((size_t)info.B, sizeof *src);
    d_plane = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    d_packed = (uint8_t**)calloc((size_t)info.B, sizeof(uint8_t*));
    h_K = (double*)malloc((size_t)info.B * 9 * sizeof(double));
    h_kitti = (double*)malloc(n_slots * 16 * sizeof(double));
    h_rec = (float*)malloc(n_slots * 32 * sizeof(float));
    h_file = (uint8_t*)malloc(file_bytes);
    if (!src || !d_plane || !d_packed || !h_K || !h_kitti || !h_rec || !h_file) { fprintf(stderr, "engine_detect_raw: out of host memory\n"); goto done; }

    in = fopen(argv[2], "rb");
    if (!in || fread(h_K, sizeof(double), (size_t)info.B * 9, in) != (size_t)info.B * 9 || fread(params.mean, sizeof(float), 3, in) != 3 ||
        fread(params.std, sizeof(float), 3, in) != 3 || fread(tail, sizeof(int32_t), 5, in) != 5 || fread(wb, sizeof(float), 3, in) != 3) {
        fprintf(stderr, "engine_detect_raw: cannot read %s\n", argv[2]);
        goto done;
    }
    fclose(in); in = NULL;
    params.resize_to = tail[0];
    if (tail[1] < 0 || tail[1] > 3) { fprintf(stderr, "engine_detect_raw: pattern %d\n", (int)tail[1]); goto done; }

    /* the sRGB transfer curve over the 4096 tone indices, rounded half up */
    for (k = 0; k < 4096; ++k) {
        const double u = k / 4095.0, v = u <= 0.0031308 ? 12.92 * u : 1.055 * pow(u, 1.0 / 2.4) - 0.055;
        h_tone[k] = (uint8_t)floor(v * 255.0 + 0.5);
    }
    HIP_OK(hipMalloc((void**)&d_tone, sizeof h_tone));
    HIP_OK(hipMemcpy(d_tone, h_tone, sizeof h_tone, hipMemcpyHostToDevice));

    for (b = 0; b < info.B; ++b) {
        in = fopen(argv[5 + b], "rb");
        if (!in || fread(h_file, 1, file_bytes, in) != file_bytes || fgetc(in) != EOF) {
            fprintf(stderr, "engine_detect_raw: %s is not a %d x %d RAW10 frame of %zu bytes\n", argv[5 + b], w, h, file_bytes);
            goto done;
        }
        fclose(in); in = NULL;
        HIP_OK(hipMalloc((void**)&d_plane[b], (size_t)pitch * h));
        HIP_OK(hipMemcpy2D(d_plane[b], (size_t)pitch, h_file, (size_t)row, (size_t)row, (size_t)h, hipMemcpyHostToDevice));
        HIP_OK(hipMalloc((void**)&d_packed[b], (size_t)h * w * 3));
        src[b].plane = d_plane[b];
        src[b].d_tone = d_tone;                                   /* the frames of one camera share a table */
        src[b].pitch = pitch; src[b].h = h; src[b].w = w;
        src[b].layout = RTM3D_RAW_MIPI10; src[b].bits = 10; src[b].pattern = tail[1];
        for (k = 0; k < 4; ++k) {
            src[b].black[k] = (uint16_t)tail[4];
            src[b].gain[k] = (uint16_t)floor((double)wb[cell_colour[tail[1]][k]] * 1024.0 + 0.5);
        }
        src[b].ccm[0] = src[b].ccm[4] = src[b].ccm[8] = 1024;
    }

    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc((void**)&d_K, (size_t)info.B * 9 * sizeof(double)));
    HIP_OK(hipMalloc((void**)&d_rec, n_slots * 32 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_kitti, n_slots * 16 * sizeof(double)));
    HIP_OK(hipMemcpy(d_K, h_K, (size_t)info.B * 9 * sizeof(double), hipMemcpyHostToDevice));
    RT_OK(rtm3d_engine_set_frame_params(ctx, &params));
    HIP_OK(hipMalloc(&d_ws, rtm3d_engine_frames_workspace_bytes(ctx)));
    RT_OK(rtm3d_engine_detect_frames_raw(ctx, stream, src, (uint8_t* const*)d_packed, tail[2], tail[3], d_K, d_rec, d_kitti, d_ws));
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(h_kitti, d_kitti, n_slots * 16 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_rec, d_rec, n_slots * 32 * sizeof(float), hipMemcpyDeviceToHost));
    printf("engine_detect_raw: %s %d RAW10 frames of %dx%d (pitch %d) on a %dx%d canvas\n", info.backbone, info.B, h, w, pitch, info.H, info.W);
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
    printf("engine_detect_raw: %d detections, %d KITTI rows\n", found, kept);
    rc = 0;
done:
    if (in) fclose(in);
    if (d_ws) (void)hipFree(d_ws);
    if (d_kitti) (void)hipFree(d_kitti);
    if (d_rec) (void)hipFree(d_rec);
    if (d_K) (void)hipFree(d_K);
    if (d_tone) (void)hipFree(d_tone);
    if (d_plane) for (b = 0; b < info.B; ++b) if (d_plane[b]) (void)hipFree(d_plane[b]);
    if (d_packed) for (b = 0; b < info.B; ++b) if (d_packed[b]) (void)hipFree(d_packed[b]);
    if (stream) (void)hipStreamDestroy(stream);
    rtm3d_ctx_destroy(ctx);
    free(src); free(d_plane); free(d_packed); free(h_K); free(h_kitti); free(h_rec); free(h_file);
    return rc;
}
