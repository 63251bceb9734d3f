/* rsd_graph.h -- C ABI of the librsd render-graph host (csrc/host/graph.h).
 *
 * This is the surface a graph script binds (Falcor's Python RenderGraph API,
 * RenderGraph.cpp / RenderGraphScripting): scripts/SVAO*.py call
 *   RenderGraph(name)              -> rsd_graph_create        (RenderGraph.cpp:55 create)
 *   g.create_pass(n, type, dict)   -> rsd_graph_create_pass   (RenderGraph.cpp:101 createPass)
 *   g.add_edge(src, dst)           -> rsd_graph_add_edge      (RenderGraph.cpp:249 addEdge)
 *   g.mark_output(name)            -> rsd_graph_mark_output   (RenderGraph.cpp:525 markOutput)
 * and the application drives it with
 *   setScene / compile / execute / getOutput / setInput
 *                                  -> rsd_graph_set_scene / _compile / _execute / _get_output / _set_input
 *                                     (RenderGraph.cpp:158, 336, 420, 470, 444)
 * Pass types come from the plugin registry (Plugin.cpp:45-91): built-ins (GuardBand,
 * GBufferRaster, LinearizeDepth, CompressNormals, StochasticDepthMapRT, SVAO), then
 * dlopen("<plugin dir>/<Type>.so") with extern "C" registerPlugin, else a no-op stub.
 * Properties travel as a flat JSON object ({"radius": 0.2, "cull": "Back", ...}).
 *
 * Every call returns rsd_status and never throws; rsd_last_error() has the message.
 */
#ifndef RSD_GRAPH_H
#define RSD_GRAPH_H
#include <stddef.h>
#include <stdint.h>

#include "rsd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsd_graph rsd_graph;

/* resource formats of graph textures (graph.h Format) */
typedef enum {
    RSD_FMT_R32F = 0, RSD_FMT_RG32F = 1, RSD_FMT_RGBA32F = 2, RSD_FMT_R16U = 3,
    RSD_FMT_R8U = 4, RSD_FMT_R8UNORM = 5, RSD_FMT_R32U = 6, RSD_FMT_UNKNOWN = 7,
    RSD_FMT_R16F = 8, RSD_FMT_RG16F = 9, RSD_FMT_RGBA16F = 10, /* StochasticDepthMapRT Use16Bit */
    RSD_FMT_RG8UNORM = 11                                      /* SVAO ao with dualAO */
} rsd_format;

typedef struct {
    void* ptr;        /* device pointer, [layer][y][x][texel] */
    uint32_t width, height, layers;
    uint32_t format;  /* rsd_format */
    uint64_t bytes;
} rsd_texture;

rsd_status rsd_graph_create(const char* name, rsd_graph** out);
void rsd_graph_destroy(rsd_graph* g);
rsd_status rsd_graph_create_pass(rsd_graph* g, const char* pass_name, const char* type, const char* props_json);
rsd_status rsd_graph_add_edge(rsd_graph* g, const char* src, const char* dst);
rsd_status rsd_graph_mark_output(rsd_graph* g, const char* name);
/* scene + camera of the frame; call again with a new camera each frame (the camera is copied) */
rsd_status rsd_graph_set_scene(rsd_graph* g, rsd_scene* scene, const rsd_camera* cam);
/* Moved geometry (rsd.h rsd_scene_update_positions) for the graph's scene, which the application uploaded with
 * rsd_scene_upload_dynamic before rsd_graph_set_scene: enqueued on `stream`, so the next rsd_graph_execute on
 * that stream renders the moved scene.  GBufferRaster.mvec follows the geometry when the scene tracks motion
 * (rsd.h rsd_scene_track_motion): the pass then renders with rsd_gbuffer_motion and snapshots the positions
 * after it ran (rsd_scene_motion_begin_frame), so the updates enqueued before the next execute are measured
 * against this frame; TemporalAO and TAA reproject with that mvec.  On a scene that does not track motion mvec
 * knows the camera's motion only.  TemporalDepthPeel does not read mvec and TemporalAO's depth-rejection test
 * transforms the previous depth with the camera alone: those know the camera's motion only. */
rsd_status rsd_graph_update_scene_positions(rsd_graph* g, const float* positions, uint32_t vertex_count,
                                            uint32_t positions_on_device, rsd_stream stream);
/* The same for a pose of the scene's rig (rsd.h rsd_scene_update_pose; the rig was attached to the scene with
 * rsd_scene_attach_rig). */
rsd_status rsd_graph_update_scene_pose(rsd_graph* g, const float* matrices, uint32_t matrix_count,
                                       uint32_t matrices_on_device, rsd_stream stream);
/* external input bound to "pass.field" (caller-owned device memory) */
rsd_status rsd_graph_set_input(rsd_graph* g, const char* name, const rsd_texture* tex);
rsd_status rsd_graph_compile(rsd_graph* g, uint32_t width, uint32_t height, rsd_stream stream);
rsd_status rsd_graph_execute(rsd_graph* g, rsd_stream stream);
/* compile without device work: culling, execution order and the resource table only
 * (RenderGraphCompiler.cpp:48-172); lets a script be validated on a host without a GPU */
rsd_status rsd_graph_plan(rsd_graph* g, uint32_t width, uint32_t height);
/* resource table of the last plan/compile: "pass.field width height layers format\n" lines */
rsd_status rsd_graph_resources(const rsd_graph* g, char* buf, size_t cap, size_t* needed);
/* "pass.field" of a compiled graph (graph-owned memory, valid until the next compile) */
rsd_status rsd_graph_get_output(rsd_graph* g, const char* name, rsd_texture* out);
/* device-to-device (or to host) copy of a graph resource, exactly its size in bytes */
rsd_status rsd_graph_copy_output(rsd_graph* g, const char* name, void* dst, uint64_t bytes, rsd_stream stream);
/* pass names in execution order, '\n'-separated; *needed receives the full length + 1 */
rsd_status rsd_graph_execution_order(const rsd_graph* g, char* buf, size_t cap, size_t* needed);
/* per-pass GPU time (ms) of the last execute, in execution order (synchronises the stream) */
rsd_status rsd_graph_pass_times(rsd_graph* g, float* ms, uint32_t cap, uint32_t* count);
/* graph dictionary entry (RenderData::getDictionary), e.g. "guardBand" */
rsd_status rsd_graph_get_dict_int(const rsd_graph* g, const char* key, int64_t* out);
rsd_status rsd_graph_pass_count(const rsd_graph* g, uint32_t* passes, uint32_t* edges);

/* --- image passes after SVAO in the graph scripts ------------------ */
/* CrossBilateralBlur (CrossBilateralBlur.ps.slang:1-88, CrossBilateralBlur.cpp:113-149):
 * R8Unorm AO -> x blur into d_pingpong -> y blur into d_dst, KERNEL_RADIUS 1..20 (default 4),
 * betterSlope (default 1); writes only inside the guard band (scissor). */
rsd_status rsd_cross_bilateral_blur(const uint8_t* d_src, const float* d_linear_z, uint32_t z_w, uint32_t z_h,
                                    uint8_t* d_pingpong, uint8_t* d_dst, uint32_t width, uint32_t height,
                                    uint32_t guard_band, uint32_t kernel_radius, uint32_t better_slope,
                                    rsd_stream stream);
/* The same for a source of src_texel_bytes-byte texels, 1 (R8Unorm) or 2 (RG8Unorm: scripts/HBAO.py blurs the
 * interleaved (bright, dark) map): the x pass reads byte 0 of each source texel, the shader's `.x`
 * (CrossBilateralBlur.ps.slang:72); d_pingpong and d_dst stay R8Unorm.  rsd_cross_bilateral_blur is this
 * with src_texel_bytes = 1. */
rsd_status rsd_cross_bilateral_blur_src(const uint8_t* d_src, uint32_t src_texel_bytes, const float* d_linear_z,
                                        uint32_t z_w, uint32_t z_h, uint8_t* d_pingpong, uint8_t* d_dst,
                                        uint32_t width, uint32_t height, uint32_t guard_band, uint32_t kernel_radius,
                                        uint32_t better_slope, rsd_stream stream);
/* AOGuidedBlur (AOGuidedBlur.ps.slang:105-208, AOGuidedBlur.cpp:121-173): resolves a (bright, dark) AO map into one
 * AO value.  d_src: `layers` layers of qw x qh texels of src_texel_bytes bytes, RG8Unorm (2) or R8Unorm (1: dark
 * reads 0); layers 16: qw x qh = ceil(width/4) x ceil(height/4) (rsd_deinterleave, rsd_hbao), layers 1: the frame
 * itself.  d_depth_layers: the linear depth in the same shape, R32F.  The x pass writes (means, meansSq) into
 * d_pingpong (RGBA8Unorm, 4 bytes per texel of d_src), the y pass the result into d_dst (R8Unorm); both write only
 * inside the scissor guard_band / int(sqrt(layers) + 0.5) of each layer, while the taps are clamped to the
 * guard band's uv bounds of the full-size width x height frame.  kernel_radius 1..20 (the pass's default 4);
 * local_deviation 1 (the shader's default) weighs by |original - mean|, 0 by sqrt|meanSq - mean^2|. */
typedef struct {
    uint32_t kernel_radius;
    uint32_t local_deviation;
    uint32_t guard_band;
    uint32_t width, height; /* the full-size frame */
    uint32_t layers;        /* 1 or 16 */
    uint32_t src_texel_bytes;
} rsd_ao_guided_blur_params;
rsd_status rsd_ao_guided_blur(const rsd_ao_guided_blur_params* params, const uint8_t* d_src,
                              const float* d_depth_layers, uint8_t* d_pingpong, uint8_t* d_dst, rsd_stream stream);
/* The AOGuidedBlur pass with enabled = False (AOGuidedBlur.cpp:130-138): the blit of the source into the R8Unorm
 * output, byte 0 of each of the `texels` source texels (all layers, no scissor). */
rsd_status rsd_ao_first_channel(const uint8_t* d_src, uint32_t src_texel_bytes, uint64_t texels, uint8_t* d_dst,
                                rsd_stream stream);
/* AOVarianceFix (AOVarianceFix.ps.slang:37-99, AOVarianceFix.cpp:115-159): the one-pass variant over the centre and
 * its four cross neighbours, through a linear / clamp sampler (librsd's 8-bit sub-texel bilinear).  d_bright, d_dark
 * and d_dst R8Unorm, d_depth_layers R32F, all `layers` layers shaped as above; the same scissor and uv bounds. */
typedef struct {
    uint32_t guard_band;
    uint32_t width, height; /* the full-size frame */
    uint32_t layers;        /* 1 or 16 */
} rsd_ao_variance_fix_params;
rsd_status rsd_ao_variance_fix(const rsd_ao_variance_fix_params* params, const uint8_t* d_bright,
                               const uint8_t* d_dark, const float* d_depth_layers, uint8_t* d_dst, rsd_stream stream);
/* RayMinMaxLength (RayMinMaxLength.ps.slang:4-16): the SD ray interval length per texel,
 * max(0, asfloat(rayMax) - asfloat(rayMin)) / 32, and 0 where rayMax is 0 (R32Float). */
rsd_status rsd_ray_min_max_length(const uint32_t* d_ray_min, const uint32_t* d_ray_max, uint32_t width,
                                  uint32_t height, float* d_out, rsd_stream stream);
/* DeinterleaveTexture (Deinterleave.slang, DeinterleaveTexture.cpp:143-158): a width x height
 * texture of texel_bytes-byte texels -> 16 layers of ceil(width/4) x ceil(height/4), layer
 * (dy * 4 + dx) holding src[4y + dy][4x + dx] (0 outside the source).  InterleaveTexture
 * (Interleave.slang): the inverse, width x height (the full-size image) from the 16 layers. */
rsd_status rsd_deinterleave(const void* d_src, uint32_t width, uint32_t height, uint32_t texel_bytes, void* d_dst,
                            rsd_stream stream);
rsd_status rsd_interleave(const void* d_src, uint32_t width, uint32_t height, uint32_t texel_bytes, void* d_dst,
                          rsd_stream stream);
/* AOFlickerMask (AOFlickerMask.cpp:73-86, AOFlickerMask.ps.slang:43-63): 1 where the pixel's
 * x and y neighbours lie in its view-space normal plane (|dot| <= 0.1), else 0 (R8Uint).
 * d_normal_w: world-space normals, RGBA32F (GBufferRaster.faceNormalW). */
rsd_status rsd_ao_flicker_mask(const float* d_linear_z, const float* d_normal_w, uint32_t width, uint32_t height,
                               const rsd_camera* cam, uint8_t* d_mask, rsd_stream stream);
/* BinaryDilation (BinaryDilation.ps.slang:13-43): min (op_max 0) or max (op_max 1) over the
 * five 2x2 Gather footprints of the pixel (R8Uint in and out, not in place). */
rsd_status rsd_binary_dilation(const uint8_t* d_in, uint32_t width, uint32_t height, uint32_t op_max, uint8_t* d_out,
                               rsd_stream stream);
/* TAA (TAA.cpp:99-124, TAA.ps.slang:78-150): colour-box clamped, motion-compensated history
 * blend.  Colours RGBA32F (the output's alpha is 1), motion vectors RG32F in uv units; the
 * caller keeps d_prev_color = the previous output (TAA.cpp:123 blit; zeros on the first frame).
 * TAA.h defaults: alpha 0.1, color_box_sigma 1.0, anti_flicker 1.  d_color_out must not alias
 * d_prev_color. */
rsd_status rsd_taa(const float* d_color_in, const float* d_mvec, const float* d_prev_color, uint32_t width,
                   uint32_t height, float alpha, float color_box_sigma, uint32_t anti_flicker, float* d_color_out,
                   rsd_stream stream);
/* TemporalAO enabled (TemporalAO.cpp:113-163, TemporalAO.ps.slang:55-101): reproject the previous
 * frame's AO along the motion vectors (RG32F, uv units), reject on > 10 % relative depth change or
 * a non-zero stable-mask pixel (d_stable_mask may be NULL: none), accumulate up to 30 frames.
 * prev_view_to_cur_view = viewMat * inverse(prevViewMat), row-major (TemporalAO.cpp:156).
 * Writes AO (R8Unorm) and the history count (R8Uint) inside the guard-band scissor; the caller
 * keeps the previous frame's linear depth, AO output and history (the pass's blits, :165-168). */
rsd_status rsd_temporal_ao(const uint8_t* d_ao_in, const float* d_linear_z, const float* d_mvec,
                           const float* d_prev_linear_z, const uint8_t* d_prev_ao, const uint8_t* d_prev_history,
                           const uint8_t* d_stable_mask, uint32_t width, uint32_t height, uint32_t guard_band,
                           const rsd_camera* cam, const float prev_view_to_cur_view[16], uint8_t* d_ao_out,
                           uint8_t* d_history_out, rsd_stream stream);
/* TemporalDepthPeel, Implementation::Iterative (TemporalDepthPeel.cpp:161-270, TemporalDepthPeel.ps.slang:
 * 319-425): the second depth layer of DualDepth SVAO (rsd_svao_params.d_depth2) without scene access.  Per
 * pixel, the view ray from linear depth + min_separation to farZ is taken into the previous frame with
 * cur_view_to_prev_view = prevViewMat * inverse(viewMat), clipped to its screen and bisected (at most
 * max_iterations steps, 0..256; the pass uses 32) against d_prev_depth2, the previous frame's output (zeros
 * on the first frame); the best sample returns through prev_view_to_cur_view = viewMat * inverse(prevViewMat).
 * It is written when it lies > depth + min_separation and < 0.99 farZ; every other pixel gets its linear depth.
 * Both matrices row-major; all images width x height R32F; d_depth2 must not alias d_prev_depth2 (the caller
 * copies the output into its history after the call, TemporalDepthPeel.cpp:264).  Exact numerics only. */
rsd_status rsd_temporal_depth_peel(const float* d_linear_z, const float* d_prev_depth2, uint32_t width,
                                   uint32_t height, const rsd_camera* cam, const float cur_view_to_prev_view[16],
                                   const float prev_view_to_cur_view[16], float min_separation,
                                   int32_t max_iterations, float* d_depth2, rsd_stream stream);
/* GBufferRaster.mvec for a static scene and a moving camera (librsd definition): the pixel-centre
 * primary hit (from the linear depth) projected with the previous camera, prevUV - uv (RG32F). */
rsd_status rsd_motion_vectors(const rsd_camera* cam, const rsd_camera* prev_cam, const float* d_linear_z,
                              uint32_t width, uint32_t height, float* d_mvec, rsd_stream stream);
/* The same from GBufferRaster's non-linear depth (the GBufferRaster pass's mvec channel): linearised
 * in-kernel like rsd_linearize_depth, background classified on the raw value (d >= 1, the cleared
 * depth, GBufferRaster.cpp:176) -> mvec (0, 0) whatever near / far do to its linearisation. */
rsd_status rsd_motion_vectors_raster(const rsd_camera* cam, const rsd_camera* prev_cam, const float* d_depth,
                                     uint32_t width, uint32_t height, float* d_mvec, rsd_stream stream);
/* ImageEquation (ImageEquation.cpp:134-160, ImageEquation.ps.slang): `formula` is the HLSL
 * expression of `float4 result = (FORMULA)` over I0..I3[xy].  Compile on the host (syntax
 * errors -> RSD_ERR_INVALID_ARG, message in rsd_last_error), run on a stream: inputs[4]
 * (ptr NULL = unbound; any rsd_format but the 16-bit float ones), output RGBA32F / RG32F / R32F / R8Unorm. */
typedef struct rsd_image_program rsd_image_program;
rsd_status rsd_image_equation_compile(const char* formula, rsd_image_program** out);
rsd_status rsd_image_equation_info(const rsd_image_program* prog, uint32_t* instructions, uint32_t* texture_mask);
rsd_status rsd_image_equation_run(const rsd_image_program* prog, const rsd_texture* inputs, const rsd_texture* out,
                                  rsd_stream stream);
void rsd_image_equation_release(rsd_image_program* prog);

/* ConvolutionalNet (ConvolutionNet.h:115-231, ConvolutionalNet.cpp:131-235): the learned resolve of the (bright, dark)
 * AO pair -- a small convolutional net per array slice over four single-channel images (bright, dark, importance,
 * depth: channels 0..3 of the first layer), ReLU between the layers, the last layer's channel 0 clamped into
 * [dark, bright].  A net is 1..8 layers for each of `slices` (1 or 16) slices; every slice has its own weights but
 * the same layer count, kernel sizes and channel counts (RSD_ERR_UNSUPPORTED otherwise, as for a kernel size outside
 * 1..7, more than 32 channels, more than 4 input channels or channels_in[l] != channels_out[l - 1]).
 * weights: [slices][K][K][Cin][Cout] with axis 0 the x offset: w[a][b] applies at (x + a - K/2, y + b - K/2), the
 * transpose of the Keras layout (what Matrix::get indexes, ConvolutionNet.h:16-24).  A tap outside the image reads 0.
 * rsd_convnet_create takes the arrays as they are; rsd_convnet_load_dir reads the reference's file layout,
 * <dir>/<slice>_weight_<l>.npy ('<f4' [K][K][Cin][Cout]) and <slice>_bias_<l>.npy ([Cout]; a missing file: zeros) for
 * l = 0.. until no weight file exists, and rounds every value to (float)strtod of its "%g" text: the reference
 * prints its weights into shader text with operator<<(float).  Both are host-only; the first rsd_convnet_run on a
 * device uploads the weights to it with hipMalloc and a synchronous hipMemcpy, so that first run must not sit inside a
 * stream capture: run the net once before capturing.  Later runs on that device only launch kernels.  Runs of one
 * net may come from several host threads; rsd_convnet_release frees the uploads and must be the net's last call, with
 * no run in flight on another thread. */
typedef struct rsd_convnet rsd_convnet;
typedef struct {
    uint32_t kernel, channels_in, channels_out;
    const float* weights; /* [slices][K][K][Cin][Cout] */
    const float* bias;    /* [slices][Cout] or NULL = zeros */
} rsd_convnet_layer;
rsd_status rsd_convnet_create(const rsd_convnet_layer* layers, uint32_t layer_count, uint32_t slices,
                              rsd_convnet** out);
rsd_status rsd_convnet_load_dir(const char* dir, uint32_t slices, rsd_convnet** out);
void rsd_convnet_release(rsd_convnet* net);
typedef struct {
    uint32_t layers, slices;
    uint32_t radius; /* sum of the layers' K / 2: how far the output depends on the inputs */
    uint32_t fused;  /* 1: a Float-precision run takes the fused kernel (its LDS footprint fits), 0: one launch per layer */
    uint32_t kernel[8], channels_in[8], channels_out[8];
} rsd_convnet_info;
rsd_status rsd_convnet_get_info(const rsd_convnet* net, rsd_convnet_info* info);
enum { RSD_CONVNET_FLOAT = 0, RSD_CONVNET_HALF = 1, RSD_CONVNET_UNORM = 2 }; /* rsd_convnet_params.precision */
/* One run.  The four inputs are `layers` layers (16: ceil(width/4) x ceil(height/4) each, 1: the frame itself) of
 * in_texel_bytes[i] = 1 (R8Unorm, byte / 255) or 4 (R32Float) bytes per texel; only the first channels_in[0] are read
 * (and bright and dark by the clamp), the others may be NULL.  d_out: R32Float in the same shape.  Every layer draws
 * only inside the scissor guard_band / int(sqrt(layers) + 0.5) of each layer (rsd_ao_guided_blur's): output texels
 * outside keep what d_out held, intermediate texels outside read 0, the inputs are read wherever the image has them.
 * precision: how an intermediate is stored between layers -- unchanged, as binary16 (round to nearest even) or as
 * R8Unorm.  clamp_output 1: min(max(v, dark), bright) (a NaN gives dark, dark > bright gives bright), 0: v.
 * numerics: RSD_NUMERICS_EXACT rounds every multiply and add separately in the reference's order (bias, then input
 * channels -- in groups of 4 after the first layer --, then y, then x, then the channel of the group); the zero
 * default RSD_NUMERICS_FAST may fuse and applies to Float only: Half and UNorm always run the exact arithmetic.
 * d_scratch: rsd_convnet_scratch_bytes bytes (may be NULL when that is 0); layer l < layers - 1 of the net keeps its
 * activations there as [slices][Cout][h][w] planes, one 256-byte-aligned block per layer in order, when the
 * per-layer kernels run.  RSD_CONVNET_FUSED=off in the environment (read by every run) forces those kernels. */
typedef struct {
    uint32_t width, height; /* the full-size frame */
    uint32_t guard_band;
    uint32_t layers;        /* 1 or 16, == the net's slices */
    uint32_t precision, clamp_output, numerics;
    uint32_t in_texel_bytes[4];
} rsd_convnet_params;
uint64_t rsd_convnet_scratch_bytes(const rsd_convnet* net, const rsd_convnet_params* params);
rsd_status rsd_convnet_run(rsd_convnet* net, const rsd_convnet_params* params, const void* d_bright,
                           const void* d_dark, const void* d_importance, const void* d_depth, void* d_scratch,
                           float* d_out, rsd_stream stream);

/* plugin registry */
rsd_status rsd_plugin_set_dir(const char* dir);
/* registered pass types, '\n'-separated */
rsd_status rsd_plugin_types(char* buf, size_t cap, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* RSD_GRAPH_H */
