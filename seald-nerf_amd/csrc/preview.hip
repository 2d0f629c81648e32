// The finishing pass of a preview frame (reference: Trainer.test_gui, SealDNeRF/utils.py:174-240 -- background mix, depth
// normalisation, nan_to_num, F.interpolate(mode='nearest') back to the window's size, linear_to_srgb, the position under every pixel
// -- and the GUI's running mean over jittered frames, SealDNeRF/gui.py:241-267), as ONE streaming launch over the output pixels, run
// after the device loop in place of sdn_render_finish.  One pixel per lane, no LDS; consecutive lanes read consecutive (or, upsampling,
// repeated) rays and write consecutive pixels.
// sdn_preview_finish_group finishes and folds the first n_fold frames of a FRAME GROUP -- the jittered samples of one view that one loop
// rendered together (DeviceLoop.render_samples) -- in the same launch: the one-frame pass is its n_fold == 1 case, every step is
// written once, and a lane folds its pixel's frames in order, in a register, with the roundings of successive one-frame calls.
#include <float.h>

#include "sdn_common.h"

namespace {

struct PreviewArgs {
    const float *image, *weights_sum, *depth, *nears, *fars, *rays_o, *rays_d;   // per ray, [n_frames * rH * rW], frame-major
    const float *bg_rays;                                                         // per ray [n_frames * rH * rW, 3], or nullptr: bg
    float bg[3];
    uint32_t rH, rW, H, W;
    float scale_y, scale_x;                                                       // (float)rH / H, (float)rW / W
    int normalize, to_srgb;
    float *image_out, *depth_out, *pos_out, *accum;
    int32_t spp;                                                                  // frames in accum before this launch
    uint32_t n_fold;                                                              // frames finished and folded by this launch (1: one frame)
};

// nerf/utils.py:44-45, the reference's constants (0.41666, not 1 / 2.4), each operation rounded on its own
__device__ __forceinline__ float linear_to_srgb(float x) { return x < 0.0031308f ? 12.92f * x : 1.055f * powf(x, 0.41666f) - 0.055f; }

__global__ void __launch_bounds__(256) k_preview_finish(PreviewArgs a) {
    const uint32_t p = threadIdx.x + blockIdx.x * blockDim.x;
    if (p >= a.H * a.W) return;
    const uint32_t y = p / a.W, x = p - y * a.W;
    // torch's `nearest`: src = min((int)floorf(dst * scale), in - 1) with scale = (float)in / out; the identity when in == out
    const uint32_t sy = min((uint32_t)floorf((float)y * a.scale_y), a.rH - 1u);
    const uint32_t sx = min((uint32_t)floorf((float)x * a.scale_x), a.rW - 1u);
    const size_t frame_rays = (size_t)a.rH * a.rW;
    const size_t q = (size_t)p * 3;
    size_t s = (size_t)sy * a.rW + sx;                        // < rH * rW; frame f's ray: + f * rH * rW < the length of every per-ray array
    float c[3], mean[3] = {0.0f, 0.0f, 0.0f}, d = 0.0f;
    for (uint32_t f = 0; f < a.n_fold; f++, s += frame_rays) {
        const float w = 1 - a.weights_sum[s];
        #pragma unroll
        for (int k = 0; k < 3; k++) {
            const float bg = a.bg_rays ? a.bg_rays[s * 3 + k] : a.bg[k];
            c[k] = a.image[s * 3 + k] + w * bg;
            if (a.to_srgb) c[k] = linear_to_srgb(c[k]);
        }
        d = a.depth[s];
        if (a.normalize) {
            const float near = a.nears[s];
            d = fmaxf(d - near, 0.0f) / (a.fars[s] - near);
        }
        // torch.nan_to_num with its defaults
        if (d != d) d = 0.0f;
        else if (d == INFINITY) d = FLT_MAX;
        else if (d == -INFINITY) d = -FLT_MAX;
        if (a.accum) {
            const float spp = (float)((uint32_t)a.spp + f);   // the count a one-frame call for frame f would be handed
            #pragma unroll
            for (int k = 0; k < 3; k++) {
                // spp == 0 overwrites: the buffer may hold anything (a NaN times zero would stay a NaN)
                const float old = f == 0 ? (spp == 0.0f ? 0.0f : a.accum[q + k]) : mean[k];
                mean[k] = spp == 0.0f ? c[k] : (old * spp + c[k]) / (spp + 1.0f);
            }
        }
    }
    s -= frame_rays;                                          // the last folded frame: its values are the launch's image, depth and position
    a.image_out[q] = c[0]; a.image_out[q + 1] = c[1]; a.image_out[q + 2] = c[2];
    a.depth_out[p] = d;
    if (a.pos_out) {   // (rH == H and rW == W: checked by the host)
        #pragma unroll
        for (int k = 0; k < 3; k++) a.pos_out[q + k] = a.rays_o[s * 3 + k] + d * a.rays_d[s * 3 + k];
    }
    if (a.accum) {
        #pragma unroll
        for (int k = 0; k < 3; k++) a.accum[q + k] = mean[k];
    }
}

// checks and launch shared by the two entry points: n_frames * rH * rW rays behind every per-ray pointer, the first n_fold frames folded
int preview_finish(const SdnRenderCtx *c, uint32_t n_frames, uint32_t n_fold, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W,
                   const float *bg_color, const float *bg_rays, int normalize, int to_srgb, float *image_out, float *depth_out, float *pos_out,
                   float *accum, int32_t spp, void *stream) {
    if (!c || !image_out || !depth_out || rH == 0 || rW == 0 || H == 0 || W == 0) return SDN_E_BADARG;
    if (!c->image || !c->weights_sum || !c->depth || (!bg_color && !bg_rays)) return SDN_E_BADARG;
    if ((uint64_t)rH * rW * n_frames != c->N || (uint64_t)H * W > (1ull << 30)) return SDN_E_BADARG;
    if (n_fold == 0 || n_fold > n_frames) return SDN_E_BADARG;
    if (normalize && !(c->nears && c->fars)) return SDN_E_BADARG;
    if (pos_out && (rH != H || rW != W || !c->rays_o || !c->rays_d)) return SDN_E_BADARG;   // the reference's expression needs one ray per pixel
    if (accum && spp < 0) return SDN_E_BADARG;
    PreviewArgs a;
    a.image = c->image; a.weights_sum = c->weights_sum; a.depth = c->depth; a.nears = c->nears; a.fars = c->fars;
    a.rays_o = c->rays_o; a.rays_d = c->rays_d; a.bg_rays = bg_rays;
    for (int k = 0; k < 3; k++) a.bg[k] = bg_color ? bg_color[k] : 0.0f;
    a.rH = rH; a.rW = rW; a.H = H; a.W = W;
    a.scale_y = (float)rH / (float)H; a.scale_x = (float)rW / (float)W;
    a.normalize = normalize; a.to_srgb = to_srgb;
    a.image_out = image_out; a.depth_out = depth_out; a.pos_out = pos_out; a.accum = accum;
    a.spp = spp; a.n_fold = n_fold;
    hipLaunchKernelGGL(k_preview_finish, dim3(sdn_div_up(H * W, 256u)), dim3(256), 0, (hipStream_t)stream, a);
    return sdn_launch_status();
}

}  // namespace

extern "C" int sdn_preview_finish(const SdnRenderCtx *c, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W, const float *bg_color,
                                  const float *bg_rays, int normalize, int to_srgb, float *image_out, float *depth_out, float *pos_out,
                                  float *accum, int32_t spp, void *stream) {
    return preview_finish(c, 1, 1, rH, rW, H, W, bg_color, bg_rays, normalize, to_srgb, image_out, depth_out, pos_out, accum, spp, stream);
}

extern "C" int sdn_preview_finish_group(const SdnRenderCtx *c, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W, const float *bg_color,
                                        const float *bg_rays, int normalize, int to_srgb, float *image_out, float *depth_out, float *pos_out,
                                        float *accum, int32_t spp, uint32_t n_fold, void *stream) {
    if (!c || c->n_group_frames < 2 || !accum) return SDN_E_BADARG;        // a group context, and a mean to fold its frames into
    if ((uint64_t)rH * rW != c->rays_per_frame) return SDN_E_BADARG;
    return preview_finish(c, c->n_group_frames, n_fold, rH, rW, H, W, bg_color, bg_rays, normalize, to_srgb, image_out, depth_out, pos_out, accum,
                          spp, stream);
}
