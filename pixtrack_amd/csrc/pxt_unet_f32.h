// fp32 forward pass of the UNet feature pyramid (pxt_unet_f32.hip): the network pixloc runs, in pixloc's precision.
// A context made by pxt_unet_create_f32 carries one of these; every pxt_unet_* entry point of pxt_unet.hip hands an
// fp32 context over to the functions below before it touches anything of the fp16 pass.
#pragma once

#include "pxt_common.h"

namespace pxt {

struct UnetF32;  // opaque: weights in fragment order, per-layer shapes, a stats scratch

int f32_create(const void* weights_host, int64_t n_bytes, UnetF32** out);
void f32_destroy(UnetF32* net);
int64_t f32_workspace_bytes_batch(const UnetF32* net, int n_images, int H, int W);
int64_t f32_workspace_bytes_pair(const UnetF32* net, const int32_t H[2], const int32_t W[2]);
int f32_forward_batch(UnetF32* net, int n_images, const void* const* images, const int32_t* image_is_u8,
                      const uint8_t* const* masks, int H, int W, float* const* out_maps, const int32_t out_cstride[3],
                      const int32_t* normalize, void* workspace, hipStream_t s);
int f32_forward_pair(UnetF32* net, const void* const* images, const int32_t* image_is_u8, const uint8_t* const* masks,
                     const int32_t H[2], const int32_t W[2], float* const* out_maps, const int32_t out_cstride[3],
                     const int32_t* normalize, void* workspace, hipStream_t s);
int f32_activation_stats(UnetF32* net, int H, int W, const void* workspace, float* stats, hipStream_t s);
int f32_layer_views(const UnetF32* net, int n_images, int H, int W, pxt_unet_layer_view* out /* [22] */);

}  // namespace pxt
