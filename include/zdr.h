/* zdr.h — C-ABI of libzdr_hip.so, the MI355X (gfx950) back end of the zdr render()/PRB hot path.
 *
 * This is the drop-in boundary: everything the reference's
 * `Scene.render_forward` / `Scene.render_backward` (/root/reference/render.py:159-199) obtain
 * from LuisaCompute — BVH build, ray traversal, the fused integrator kernels, in-kernel
 * autodiff and the float atomic scatter — sits behind these entry points.  Plain pointers and
 * sizes only; no torch types.  Device pointers are BORROWED for the duration of a call; work
 * is enqueued on `stream` (a hipStream_t, NULL = the default stream) and NOT synchronised:
 * the caller decides when to wait (the reference synchronises on both sides, render.py:165,172).
 *
 * All functions return 0 on success or a negative ZDR_E_* code; zdr_last_error() gives the
 * thread-local message.  One in-flight call per scene handle (render.py:216-222: the
 * reference scene is not re-entrant either) — the handle owns per-call workspaces (staging cells, chunk
 * partials, work counters, the parked-vertex FIFOs), so two renders of ONE scene must not overlap, not even on
 * different streams: enqueue them on one stream, or use one scene handle per stream.
 *
 * Stream capture (hipStreamBeginCapture / torch.cuda.graph).  The render calls only enqueue, so a call made while its stream is
 * capturing is recorded into the graph — provided one eager call of the same kind, resolution and spp has sized the handle's
 * workspaces before (a call that would have to allocate while capturing returns ZDR_E_UNSUPPORTED).  A graph names the handle's
 * workspaces and everything of the scene at capture time (camera, lights, environment, sampler tables, seed are frozen into the
 * kernel arguments).  From the first captured call on the handle therefore (a) never frees a device buffer before
 * zdr_scene_destroy — one that must grow is replaced and the old one kept alive for the graphs that name it — and (b) rebuilds
 * the camera-ray tile masks in every call, captured or eager, because a replay rewrites them for its own view.  Eager calls of
 * any view or size and any number of captures may thus be interleaved with replays on the handle's stream; what still holds is
 * the rule above: one call (or replay) in flight per handle.  Destroy the graphs before the handle.
 */
#ifndef ZDR_H
#define ZDR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZDR_VERSION_STRING "zdr-mi355x 0.3 (gfx950)"
/* Bumped whenever a struct of this header changes size or meaning, or an existing entry point changes (2: tile shard + prb_mode fields;
 * 3: struct_size; 4: environment-map gradient).  A binding asserts zdr_abi_version() == ZDR_ABI_VERSION of the header it was written against.
 * Entry points that are purely added keep the version: a binding finds them by symbol (the emission gradient, zdr_scene_set_emission_values
 * and zdr_render_backward*_emission, came to version 4 that way). */
#define ZDR_ABI_VERSION 4

enum { ZDR_OK = 0, ZDR_E_INVALID = -1, ZDR_E_HIP = -2, ZDR_E_UNSUPPORTED = -3, ZDR_E_NOMEM = -4 };

/* integrators = render.py:65-69; ZDR_UVGRAD = render_duvdxy's kernel (uvgrad.py:76-98, forward only:
 * the image receives (dudx, dvdx, dudy, dvdy) per pixel) */
enum { ZDR_COLLOCATED = 0, ZDR_DIRECT = 1, ZDR_PATH = 2, ZDR_UVGRAD = 3 };
/* samplers = integrator.py:16-17 (corrmj.py is self-contained; pmj02bn.py needs tables) */
enum { ZDR_SAMPLER_CMJ = 0, ZDR_SAMPLER_PMJ02BN = 1 };
/* acceleration structure used for LuisaCompute's Accel (render.py:74,109,127) */
enum { ZDR_ACCEL_AUTO = 0, ZDR_ACCEL_BRUTE = 1, ZDR_ACCEL_BVH = 2 };
enum { ZDR_PRB_EXPECTATION = 0, ZDR_PRB_DETACHED = 1, ZDR_PRB_LITERAL = 2 };
/* most materials one zdr_render_*_materials call takes */
#define ZDR_MAX_MATERIALS 16

typedef struct zdr_scene zdr_scene;

/* render.py:28 — Camera = StructType(fov, origin, target, up); fov = full horizontal angle (rad) */
typedef struct {
    float fov;
    float origin[3], target[3], up[3];
} zdr_camera;

/* Arguments of one kernel dispatch (integrator.py:10-11, render.py:168-171,193-196) plus the
 * shard this call covers: a pixel rectangle and a sample-index range. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_render_params) of the caller's header; a mismatch is ZDR_E_INVALID */
    int32_t integrator;                /* ZDR_COLLOCATED | ZDR_DIRECT | ZDR_PATH */
    int32_t sampler;                   /* ZDR_SAMPLER_* */
    int32_t width, height;             /* res = (W, H); image tensor is (H, W, 4) */
    uint32_t spp, seed;                /* backward: the caller passes seed + 1 (render.py:196) */
    int32_t use_tent;                  /* scene.use_tent_filter (render.py:71) */
    int32_t x0, y0, x1, y1;            /* pixels [x0,x1) x [y0,y1) are rendered, others untouched */
    uint32_t sample_begin, sample_end; /* sample indices [begin,end) of [0,spp) are evaluated */
    int32_t max_depth, rr_depth;       /* prb.py:15-16: 16, 2 */
    zdr_camera camera;
    int32_t tex_h, tex_w;              /* material tensor is (tex_h, tex_w, 4) float32 */
    /* Interleaved pixel-tile shard (BASELINE configs[3] "pixel-tiled across 8 GPUs"): the rectangle is cut
     * into 8x8 tiles numbered row by row from its own corner, row r starting at column r (mod the row length) — so that
     * the tiles of one shard run along diagonals, not down the columns of the image — and this call renders the tiles
     * whose number is congruent to tile_shard_index modulo tile_shard_count: one launch per rank, every rank sees every
     * part of the image (load balance).  The shards of one count partition the rectangle.  tile_shard_count <= 1: the
     * whole rectangle. */
    int32_t tile_shard_index, tile_shard_count;
    /* Form of the PRB adjoint (backward of the path integrator only).  ZDR_PRB_EXPECTATION (0, default): the derivative of
     * the forward's expectation, which is what finite differences of render() measure (BASELINE.json's gradient bar) —
     * Russian roulette without an upper clamp (prb.py:83) makes the expectation depend on the roulette probabilities and
     * on the MIS weights, and this form differentiates through them.  ZDR_PRB_DETACHED (1): every roulette factor and MIS
     * weight held constant, which is what the reference's autodiff blocks compute (prb.py:138-146, 157-163, with the
     * corrected BSDF weight of SURVEY App. B-3).  ZDR_PRB_LITERAL (2): as DETACHED but with the BSDF-sample adjoint seeded
     * exactly as prb.py:157-163 writes it, backward(bsdf, beta / pdf_bsdf * Le * le_grad) with Le the remaining path
     * radiance — which already contains beta * bsdf / pdf, so this is NOT the derivative of the forward (19 % off finite
     * differences, tests/test_oracle_render.py); it exists so that the one output the reference defines and the other two
     * modes cannot produce is available for comparison. */
    int32_t prb_mode;
} zdr_render_params;

typedef struct {
    uint32_t ntris, nverts, ninst, light_count;
    int32_t accel;                     /* ZDR_ACCEL_BRUTE or ZDR_ACCEL_BVH actually in use */
    uint32_t bvh_nodes, bvh_max_depth, bvh_stack_entries;   /* BVH4 nodes, depth of the binary SAH tree, traversal-stack entries per lane the tree can need (the first 6-12 in LDS, the rest in scratch) */
    int32_t device;
    uint64_t device_bytes;             /* HBM held by the scene */
} zdr_scene_info_t;

const char *zdr_version(void);
int zdr_abi_version(void);             /* ZDR_ABI_VERSION the library was built with */
const char *zdr_last_error(void);

/* Replaces Scene.load_geometry (render.py:73-128): luisa.Buffer uploads, accel.add(vb, tb,
 * transform), heap.emplace(...), accel.update().  HOST inputs:
 *   verts8          nverts x 8 float32  {v[3], vt[2], vn[3]} in object space (vertex.py:4)
 *   tris            ntris  x 3 int32    indices into verts8
 *   inst_tri_begin  ninst + 1 int32     triangles [begin[i], begin[i+1]) belong to instance i
 *   inst_xform      ninst x 16 float32  row-major object->world 4x4 (NULL = identity)
 *   inst_emission   ninst x 3 float32   (render.py:85-91; a light is any emission component > 0)
 * zdr_render_forward / zdr_render_backward texture instance 0 only; every other instance is an emitter or a blocker (prb.py:45).
 * To shade several instances, each with a material of its own, see zdr_scene_set_material_slots and zdr_render_*_materials.
 * Positions: every WORLD-space position (inst_xform x v, in float32) of a vertex a triangle uses must be finite and at most
 * ZDR_MAX_COORD = 2^30 in each coordinate's magnitude — the largest power of two for which nothing the host derives from the
 * positions (plane records, normals, areas, the BVH's boxes and costs) can overflow float32; the derivation is at position_ok in
 * csrc/zdr_api.cpp.  Otherwise ZDR_E_INVALID, before any device is touched, and zdr_last_error() names the first offending instance
 * and vertex.  The limit keeps the arithmetic finite, not accurate: the error of a hit distance grows with |position|, that of a
 * barycentric with |position| / edge length ("Ray queries away from the origin"), so keep scenes near the origin.
 * A triangle without area (three equal or collinear corners) is legal and is never hit by any ray query; as part of a light it is
 * not supported. */
#define ZDR_MAX_COORD 1073741824.0f    /* 2^30 */
int zdr_scene_create(const float *verts8, uint32_t nverts, const int32_t *tris, uint32_t ntris,
                     const int32_t *inst_tri_begin, const float *inst_xform, const float *inst_emission,
                     uint32_t ninst, int device, int accel, zdr_scene **out);
int zdr_scene_destroy(zdr_scene *scene);
int zdr_scene_info(const zdr_scene *scene, zdr_scene_info_t *info);

/* Replaces Scene.update_lights (render.py:130-148). HOST input ninst x 3; rebuilds the light list. */
int zdr_scene_set_emissions(zdr_scene *scene, const float *inst_emission, void *stream);

/* Rewrites the emission VALUES of the current light list in place: emission is DEVICE float32, ninst x 3, and the rows of the instances
 * that are lights now (the list of zdr_scene_create or of the last zdr_scene_set_emissions) replace those lights' emissions everywhere the
 * kernels read them.  Rows of other instances are ignored, and those instances are left alone: the light list, light_count and every buffer
 * stay as they are.  Done by a kernel: stream-ordered, no synchronise, no reallocation, so the call can be captured and graphs keep their
 * pointers.  A component may be zero or negative; a light whose components are ALL <= 0 stays in the list (it is still picked by the light
 * sampling) but the kernels stop treating its surface as an emitter, as they do for any instance without a positive component.
 * zdr_scene_set_emissions replaces all of it, list included. */
int zdr_scene_set_emission_values(zdr_scene *scene, const float *emission, void *stream);

/* Replaces Scene.add_envmap / load_envmap (render.py:150-156, envmap.py:116-203): a lat-long environment
 * light.  HOST inputs, copied to the device: tex (tex_h x tex_w x 4 float32, already made square as
 * envmap.py:123-128 does) and the importance-sampling tables the host builds from it (zdr_amd/envmap.py:
 * alias_prob / alias_idx hold the marginal p(y) table (map_h entries) followed by map_h conditional p(x|y)
 * tables of map_w entries; pdf is map_h x map_w).  tex == NULL removes the environment (env_count = 0). */
int zdr_scene_set_envmap(zdr_scene *scene, const float *tex, uint32_t tex_h, uint32_t tex_w, const float *alias_prob,
                         const int32_t *alias_idx, const float *pdf, uint32_t map_w, uint32_t map_h);

/* Replaces the environment map's texels in place, keeping its size and its importance-sampling tables (those of the last
 * zdr_scene_set_envmap): tex is DEVICE float32, env_h x env_w x 4 as given to zdr_scene_set_envmap (already square).  The copy is
 * stream-ordered and done by a kernel, and the scene's texture buffer is never reallocated: a captured call records the copy, and
 * graphs that read the map keep reading the same buffer.  tex must be 16-byte aligned (the copy moves one float4 texel per load;
 * hipMalloc'ed memory is).  ZDR_E_INVALID when no environment map is set or tex is misaligned. */
int zdr_scene_set_envmap_texture(zdr_scene *scene, const float *tex, void *stream);

/* Rebuilds the importance-sampling tables (alias_prob, alias_idx, pdf) on the device from the environment texture as it is on `stream`,
 * after an earlier zdr_scene_set_envmap_texture on that stream for instance: the device form of what the host does before
 * zdr_scene_set_envmap (zdr_amd/envmap.py, build_tables; compensate_mis != 0 subtracts the map's mean, row by row, and clamps at 0).
 * In place and stream-ordered: no host copy, no synchronisation, and pointers and sizes stay as they are, so the call can be captured and
 * graphs captured earlier read the new tables.  Two calls on the same texture give the same bytes.  An entry whose weight is 0 in a table
 * with a positive total gets probability 0 and is nobody's alias: a texel whose pdf is 0 is never drawn.  The sample map must be the
 * 512 x 256 one (ZDR_E_UNSUPPORTED otherwise).  The first call on a handle allocates about 0.5 MiB of workspace, kept until
 * zdr_scene_destroy: made while the stream is capturing it is refused (ZDR_E_INVALID: call once before capturing).
 * ZDR_E_INVALID when no environment map is set. */
int zdr_scene_update_envmap_sampling(zdr_scene *scene, int compensate_mis, void *stream);

/* Copies the importance-sampling tables to HOST arrays in the layout of zdr_scene_set_envmap (alias_prob / alias_idx: map_h + map_h x map_w
 * entries, the marginal table first, then the rows; pdf: map_h x map_w) and synchronises `stream`.  For tests, and for handing the tables
 * to another renderer.  ZDR_E_INVALID when no environment map is set. */
int zdr_scene_get_envmap_sampling(zdr_scene *scene, float *alias_prob, int32_t *alias_idx, float *pdf, void *stream);

/* Tables of the PMJ02bn sampler (pmj02bn.py:9-18; the reference's own are absent,
 * .MISSING_LARGE_BLOBS).  HOST inputs, copied to the device: pmj [nsets][nsamples][2] uint32
 * (value / 2^32), bn [ntex][res][res] uint16 (value / 2^16). */
int zdr_scene_set_pmj02bn_tables(zdr_scene *scene, const uint32_t *pmj, uint32_t nsets, uint32_t nsamples,
                                 const uint16_t *bn, uint32_t ntex, uint32_t bnres);

/* Replaces Scene.render_forward (render.py:159-173) = render_{path,direct,collocated}_kernel
 * (integrator.py:9-30).  material: DEVICE (tex_h, tex_w, 4) float32; image: DEVICE (H, W, 4)
 * float32, pixels of the shard are overwritten with (sum over the sample range / spp,
 * (sample_end - sample_begin) / spp). */
int zdr_render_forward(zdr_scene *scene, const zdr_render_params *params, const float *material,
                       float *image, void *stream);

/* Replaces Scene.render_backward (render.py:176-199) = render_*_backward_kernel
 * (integrator.py:33-53): d_material (DEVICE, tex_h x tex_w x 4) is ACCUMULATED into (+=), as the
 * reference's atomic_fetch_add does (interaction.py:63-70); the caller zeroes it (render.py:220).
 * d_image: DEVICE (H, W, 4) cotangent of the image. */
int zdr_render_backward(zdr_scene *scene, const zdr_render_params *params, const float *d_image,
                        const float *material, float *d_material, void *stream);

/* Material slots (the reference shades one material only: its instances > 0 are lights or blockers, prb.py:45).  inst_slot (HOST,
 * ninst int32) gives each instance a material index k >= 0 of the zdr_render_*_materials calls, or -1 for none; copied to the
 * device (a cold path, like zdr_scene_set_emissions: the stream is synchronised).  What an instance does in those calls:
 *   path        slot >= 0: shaded by material k (an emitting instance still ends the path as a light, prb.py:39-46);
 *               -1: what instances > 0 do in zdr_render_forward (emitter or blocker)
 *   direct      slot >= 0: shaded by material k;  -1: returns its emission (direct.py:30-32)
 *   collocated  slot >= 0: shaded by material k;  -1: black
 * zdr_render_forward / zdr_render_backward are not affected.  Until the first call every slot is -1. */
int zdr_scene_set_material_slots(zdr_scene *scene, const int32_t *inst_slot, void *stream);

/* zdr_render_forward with one material per slot.  materials: DEVICE float32, the nmat textures concatenated texel by texel
 * (material k is dims[2k] x dims[2k+1] x 4, CLAMP bilinear as read_bsdf); dims: HOST int32 nmat x {h, w}, 1 <= nmat <=
 * ZDR_MAX_MATERIALS, every dimension >= 1.  params->tex_h / tex_w are ignored.  A slot >= nmat is ZDR_E_INVALID.  The table of
 * materials travels in the kernel arguments, so a captured call keeps the layout it was recorded with. */
int zdr_render_forward_materials(zdr_scene *scene, const zdr_render_params *params, const float *materials, const int32_t *dims,
                                 uint32_t nmat, float *image, void *stream);

/* zdr_render_backward with one material per slot: d_materials (DEVICE, packed like materials) is ACCUMULATED into (+=); each
 * material receives the gradient of the vertices shaded with it.  Staging cells are sized for all materials together. */
int zdr_render_backward_materials(zdr_scene *scene, const zdr_render_params *params, const float *d_image, const float *materials,
                                  const int32_t *dims, uint32_t nmat, float *d_materials, void *stream);

/* zdr_render_backward / zdr_render_backward_materials that also differentiate with respect to the environment map: d_env (DEVICE,
 * env_h x env_w x 4 float32, the map's size as set) is ACCUMULATED into (+=) like d_material.  The gradient is exact for the forward in
 * every prb_mode: the importance-sampling tables are held fixed, and neither Russian roulette nor the MIS weights read the map's values,
 * so each term of the estimator that reads the map (a path or camera ray that escapes, a light sample on the environment) is a weight
 * times a bilinear lookup, and its gradient is that weight times the pixel's cotangent at the lookup's four texels.  Alpha receives 0.
 * A term whose gradient is NaN is dropped on its own; a path whose radiance turns NaN later (the forward drops that sample) keeps the
 * environment terms it met before.  ZDR_E_INVALID when d_env is given and no environment map is set, whatever the integrator.
 * Otherwise d_env == NULL behaves exactly like the sibling call, and so does ZDR_COLLOCATED, which has no environment term and
 * leaves d_env untouched.  The map's staging cells have copies of their own (up to 2^22 cells in all), zeroed and gathered per call.  Runs in the
 * material-table kernels (a single material is a table of one, instance 0 shading with it), so the material gradient equals the
 * sibling's up to the order of float atomics; the _materials form takes at most ZDR_MAX_MATERIALS - 1 materials. */
int zdr_render_backward_env(zdr_scene *scene, const zdr_render_params *params, const float *d_image, const float *material,
                            float *d_material, float *d_env, void *stream);
int zdr_render_backward_materials_env(zdr_scene *scene, const zdr_render_params *params, const float *d_image, const float *materials,
                                      const int32_t *dims, uint32_t nmat, float *d_materials, float *d_env, void *stream);

/* zdr_render_backward / zdr_render_backward_materials that also differentiate with respect to the lights' emissions: d_emission (DEVICE,
 * ninst x 3 float32) is ACCUMULATED into (+=); the rows of instances outside the current light list receive nothing.  With the light list
 * fixed nothing a path decides reads an emission value (the light pick is uniform over light_count, the MIS weights read pdfs, Russian
 * roulette reads the throughput), so the forward of one seed is linear in the emissions and each term that reads one — a camera, BSDF-sample
 * or continuation ray that ends on a light, a light sample on a mesh light that is seen from its front and unoccluded — adds its weight
 * times the pixel's cotangent.  The gradient is therefore exact for the forward of the same seed in every prb_mode AS LONG AS EVERY LIGHT
 * KEEPS AT LEAST ONE POSITIVE COMPONENT (not checked: that would take a synchronise).  A light that is zero or negative in every component is
 * outside that guarantee: the forward stops treating its surface as an emitter, and the BVH kernels skip the shadow ray of a light sample
 * that carries no radiance.  The clamp of a sample's radiance to [0, 1e5] is not differentiated, as for the other gradients; a term whose
 * gradient is NaN is dropped on its own.  d_emission == NULL behaves exactly like the sibling call, and so does ZDR_COLLOCATED, which reads
 * no emission and leaves d_emission untouched; so does a scene without lights.  Not together with an environment-map gradient (there is no
 * call for both).  A wave sums its terms in LDS, per light, for the first 10 lights of the list; terms of further lights go to memory one by
 * one (correct, slower).  Runs in the material-table kernels (a single material is a table of one, instance 0 shading with it), so the
 * material gradient equals the sibling's up to the order of float atomics. */
int zdr_render_backward_emission(zdr_scene *scene, const zdr_render_params *params, const float *d_image, const float *material,
                                 float *d_material, float *d_emission, void *stream);
int zdr_render_backward_materials_emission(zdr_scene *scene, const zdr_render_params *params, const float *d_image, const float *materials,
                                           const int32_t *dims, uint32_t nmat, float *d_materials, float *d_emission, void *stream);

/* First-hit feature buffers: what each pixel SEES, rendered with the camera samples of zdr_render_forward of the same seed (not seed + 1:
 * the buffers line up with the forward image), and their adjoint with respect to the materials.  For pixel (x, y) and sample s in [0, spp):
 *   camera ray   the one zdr_render_forward draws: sampler of (x, y, s), its first 2-D draw is the jitter, tent-warped when use_tent is on
 *   first hit    the closest hit in (0, 1e30); no facing test, a surface seen from behind is still a hit
 *   interaction  p, uv, ns (normalised interpolated normal, not flipped), instance and t of that hit
 *   slot         the instance's entry in the table of zdr_scene_set_material_slots, -1 = none
 * With Hs the samples of the pixel that hit, a pixel holds ZDR_AOV_CHANNELS floats (four float4), the tensor is (H, W, 16):
 *   floats 0..2, 3     albedo, roughness     (1/spp) sum over s in Hs with slot >= 0 of read_bsdf(material[slot], uv_s), all four channels
 *   floats 4..6, 7     normal, depth         (1/spp) sum over Hs of ns_s;  (1/spp) sum over Hs of t_s
 *   floats 8..10, 11   position, coverage    (1/spp) sum over Hs of p_s;  |Hs| / spp
 *   floats 12..13      uv                    (1/spp) sum over Hs of uv_s
 *   floats 14, 15      instance, slot        of the hit with the lowest sample index, as floats; -1 when Hs is empty
 * Every averaged channel is premultiplied by coverage (a miss adds 0; divide by coverage for the mean over the hits).  The sums run in
 * sample order in float32 and are divided by (float)spp with an IEEE division; a sample with a NaN in any summed value is dropped whole.
 * params->integrator, max_depth, rr_depth, prb_mode and tex_h / tex_w are ignored: a scene of any integrator gives the same buffers.
 * The pixel rectangle and the tile shard are honoured (pixels outside keep their value); a sample range other than [0, spp) is
 * ZDR_E_UNSUPPORTED, the instance channel having no partial form.  materials, dims, nmat: as zdr_render_forward_materials.
 *
 * zdr_render_aovs_backward: only floats 0..3 depend on the materials, and linearly.  d_materials (DEVICE, packed like materials) is
 * ACCUMULATED into (+=):  d_materials[slot] += sum over s in Hs with slot >= 0 of bilinear_weights(uv_s) d_aovs[pixel, 0..3] / spp.
 * Floats 4..15 of d_aovs are not read; a cotangent with a NaN counts as 0.  The SAME seed as the forward: this is the exact transpose
 * of the forward, there is no seed + 1 here.  Both calls only enqueue and follow the stream-capture rules above. */
#define ZDR_AOV_CHANNELS 16
int zdr_render_aovs(zdr_scene *scene, const zdr_render_params *params, const float *materials, const int32_t *dims, uint32_t nmat,
                    float *aovs /* DEVICE H x W x 16 */, void *stream);
int zdr_render_aovs_backward(zdr_scene *scene, const zdr_render_params *params, const float *d_aovs /* DEVICE H x W x 16 */,
                             const float *materials, const int32_t *dims, uint32_t nmat, float *d_materials, void *stream);

/* Feature-guided à-trous denoiser: an edge-stopping wavelet filter of an (H, W, 4) image guided by the (H, W, 16) feature buffers of
 * zdr_render_aovs rendered with the same camera samples, and its adjoint with respect to the image.  No scene handle.
 * Guides of pixel p with feature row A:  c = A[11] (coverage);  if c > 0:  n = A[4..6] / c,  z = A[7] / c,  a = A[0..2] / c;  otherwise
 * n = 0, z = 0, a = 0;  id = A[14] (-1 where nothing was hit).
 * Weights, with b = (1/16, 1/4, 3/8, 1/4, 1/16), level l = 0 .. levels - 1, s = 2^l and q = p + s (i, j), i, j in {-2 .. 2}:
 *   w_l(p, q) = b[i + 2] b[j + 2] [id_p == id_q] exp(-(Tn + Tz + Ta))
 *   Tn = |n_p - n_q|^2 / sigma_normal^2
 *   Tz = (z_p - z_q)^2 / ((sigma_depth (z_p + z_q) / 2)^2 + 1e-20)            (relative depth)
 *   Ta = |a_p - a_q|^2 / sigma_albedo^2
 * A term whose sigma is <= 0 is switched off (contributes 0).  Taps outside the image do not exist.  w is symmetric in (p, q) and
 * w(p, p) = 9/64, so the normaliser below is never 0.
 * Forward:  x_0 = image, all four channels alike;  x_{l+1}(p) = sum_q w_l(p, q) x_l(q) / D_l(p),  D_l(p) = sum_q w_l(p, q);  out = x_levels.
 * The guides always come from the given feature buffers, never from a filtered level: each level is a fixed linear map
 * K_l = D_l^-1 W_l of the image, and a constant image (alpha = 1) stays constant.
 * Adjoint:  d_image = K_0^T ... K_{levels-1}^T d_out,  (K_l^T g)(q) = sum_p w_l(p, q) g(p) / D_l(p): by the symmetry of w a gather over
 * the same 25 taps of g / D_l, without atomics, bit-identical from run to run.  The feature buffers receive NO gradient: the
 * edge-stopping weights are held fixed.  Inputs are assumed finite; nothing is checked for NaN.
 *
 * All pointers are DEVICE pointers, 16-byte aligned; aovs is H x W x 16, image / out / d_out / d_image are H x W x 4.  The caller
 * provides `workspace`, at least zdr_denoise_workspace_bytes(params) bytes (0 = invalid params; grows with the size, and does not
 * shrink with the levels).  Both calls only enqueue on `stream`: they never allocate and never synchronise, so they can be captured
 * in a HIP graph without a call before.  Neither call reads what an earlier call left in the workspace — each packs the guides and
 * computes the normalisers it needs itself — so zdr_denoise_backward needs no forward call before it, and one workspace may serve
 * calls of any parameters it is large enough for, one call in flight at a time.  out and d_image are overwritten (not accumulated
 * into) and must not overlap the inputs or the workspace.
 * ZDR_E_INVALID: struct_size other than sizeof(zdr_denoise_params), levels outside 1 .. ZDR_DENOISE_MAX_LEVELS, a width or height
 * <= 0, a null or misaligned pointer, an output that overlaps an input or the workspace, a workspace that overlaps an input (byte
 * ranges as the parameters size them).  ZDR_E_UNSUPPORTED: more than 2^30 pixels.  Any other width and height >= 1 is taken. */
#define ZDR_DENOISE_MAX_LEVELS 6
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_denoise_params) */
    int32_t width, height, levels;
    float sigma_normal, sigma_depth, sigma_albedo;
} zdr_denoise_params;
size_t zdr_denoise_workspace_bytes(const zdr_denoise_params *params);
int zdr_denoise(const zdr_denoise_params *params, const float *aovs, const float *image, float *out, void *workspace, void *stream);
int zdr_denoise_backward(const zdr_denoise_params *params, const float *aovs, const float *d_out, float *d_image, void *workspace,
                         void *stream);

/* Texture-space feature buffers: what each TEXEL of a material is, where the screen-side buffers of zdr_render_aovs say what each pixel
 * sees.  The models are rasterised into the texture: which texels lie on a model, which a lookup can ever read (and so can ever receive
 * gradient), where a texel sits in the world, what its normal is and how much surface it stands for.  The layout is that of
 * zdr_render_aovs, so zdr_denoise takes the buffers as guides: a chart-aware filter of a material or of its gradient.
 *
 * Material, size, pixel space.  The call takes a material index m and a texture size tex_h x tex_w.  Pixel space is that of read_bsdf /
 * tex_footprint (csrc/scene.h): X = u (tex_w - 1), Y = (1 - v) (tex_h - 1), computed in float32 as those products.  Texel (x, y) is the
 * lattice point (x, y).
 * Triangles.  The triangles of m are those of every instance whose entry in the table of zdr_scene_set_material_slots is m (never set:
 * every entry is -1 and the buffers are empty).  Each has a global input index g = inst_tri_begin[inst] + prim.
 * coverage(x, y) = 1 iff the lattice point lies in the closed pixel-space triangle of some triangle of m, of either winding.  The test is
 * watertight: the edge function of an edge is evaluated with its two endpoints in canonical order (lexicographic on (X, Y)) and the caller
 * flips the sign, without contraction, so that two triangles that share an edge compute the same float and disagree in sign only; a lattice
 * point on a shared edge is claimed by at least one of them.  The winner is the covering triangle with the lowest g.
 * reach(x, y) = 1 iff the closed box [x - 1, x + 1] x [y - 1, y + 1] meets the closed triangle of some triangle of m (a separating-axis
 * test with the two box axes and the three edge normals), or the texel is covered: the texels a bilinear lookup somewhere on the triangle
 * can read, conservative only on a rim of measure zero where the weight is exactly 0.  The reach winner is the lowest g among the reaching
 * triangles.  coverage is a subset of reach.
 * Degenerate triangles.  A triangle with a NaN pixel-space coordinate is skipped.  One whose pixel-space area (the edge function of the side
 * opposite corner 0, at corner 0) is 0 or NaN gives no coverage, and reach by the bounding-box part of the test alone (conservative).  A
 * 1 x 1 texture makes every triangle degenerate: reach 1, coverage 0.
 * UVs outside [0, 1] are NOT clamped: the bounding box is clipped to the texture and what falls outside is ignored.  Limitation: the CLAMP
 * addressing of lookups out there, which folds them onto the border texels, is not modelled.
 * Sample point.  A covered texel: the lattice point, with barycentrics = the three edge functions over their sum, in the coverage winner.
 * A texel that is only reached: the closest point, Euclidean in pixel space, of the reach winner's closed triangle (the nearest of the
 * closest points of its three sides; barycentrics (1 - t, t) along that side).  A degenerate winner: its corner 0.  Attributes are
 * interpolated as surface_interact does: (a0 w0 + a1 w1) + a2 w2, the normal normalised afterwards.
 * A texel holds ZDR_AOV_CHANNELS floats, the tensor is (tex_h, tex_w, 16):
 *   floats 0..3        0 (no material is read: the buffers depend on the geometry and the slot table only)
 *   floats 4..6, 7     normal, texel_size    normalised interpolated normal at the sample point;  world length of one texel,
 *                                            sqrt(world area / pixel-space area) of the winner, 0 for a degenerate winner
 *   floats 8..10, 11   position, coverage    world position at the sample point;  0 or 1
 *   floats 12, 13      reach, -              0 or 1;  0
 *   floats 14, 15      instance, slot        the winner's instance and m, as floats;  -1 and -1 where reach = 0 (every other float is 0 there)
 * Float 7 sits where the screen buffers hold depth: zdr_denoise's relative-depth term then keeps texels of very different density apart
 * (sigma_depth = 0 switches it off).  zdr_denoise reads float 11 as coverage: copy float 12 there to let reached-only texels take part.
 * The result is bit-identical from run to run and between ZDR_ACCEL_BRUTE and ZDR_ACCEL_BVH (the key is g, not the slot).
 *
 * aovs (DEVICE, tex_h x tex_w x 16) is overwritten.  The caller provides `workspace`, zdr_texel_aovs_workspace_bytes(tex_h, tex_w) bytes
 * (0 = invalid size).  Three launches on `stream` — clear the keys, rasterise with atomicMin of g, resolve — that never allocate and never
 * synchronise, so the call can be captured in a HIP graph without a call before.  The scene is only read.
 * ZDR_E_INVALID: a null or misaligned (16 bytes) pointer, a size <= 0, material outside 0 .. ZDR_MAX_MATERIALS - 1, an output that overlaps
 * the workspace.  ZDR_E_UNSUPPORTED: more than 2^26 texels, or a dimension above 2^24.  A material that no instance has gives all-empty
 * buffers; it is not an error. */
size_t zdr_texel_aovs_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_scene_texel_aovs(zdr_scene *scene, int32_t material, int32_t tex_h, int32_t tex_w,
                         float *aovs /* DEVICE tex_h x tex_w x 16 */, void *workspace, void *stream);

/* UV tangents: how the texture's pixel lattice lies on the surface.  Per texel of material m, tangents (DEVICE, tex_h x tex_w x 8,
 * overwritten) holds the world derivatives of the position per texture pixel, of the texel's winner — the very winner of
 * zdr_scene_texel_aovs: the coverage winner, else the reach winner.  They are constant over a triangle, so a texel that is only reached
 * takes its reach winner's, as it takes that winner's texel_size.
 * World corners P0, P1, P2: the winner's, in input order; pixel-space corners (X_i, Y_i): the float32 products of zdr_scene_texel_aovs.
 * In float32, uncontracted, divisions and roots IEEE, per component c of a vector, dot products from x to z:
 *   e1 = P1 - P0,  e2 = P2 - P0,  a1 = X1 - X0,  a2 = X2 - X0,  b1 = Y1 - Y0,  b2 = Y2 - Y0,  det = a1 b2 - a2 b1
 *   Tx.c = (e1.c b2 - e2.c b1) / det        dp/dX: world units per texture pixel to the right
 *   Ty.c = (e2.c a1 - e1.c a2) / det        dp/dY: per texture pixel DOWNWARDS (Y = (1 - v) (tex_h - 1))
 *   C = Tx x Ty = (Tx.y Ty.z - Tx.z Ty.y, Tx.z Ty.x - Tx.x Ty.z, Tx.x Ty.y - Tx.y Ty.x),  area = sqrt(C.C),  s = C.n
 * with n the texel's normal as zdr_scene_texel_aovs wrote it (floats 4..6 of its row).  A row:
 *   floats 0..2, 3     Tx, area          area: the world area of one texel, texel_size^2 up to rounding
 *   floats 4..6, 7     Ty, orientation   +1 where s > 0, -1 where s < 0, 0 otherwise (s is 0 or NaN); a mirrored chart has the other sign
 * Eight zeros where the texel is not reached; where the winner is degenerate by zdr_scene_texel_aovs's rule — the same test on the same
 * float, so that on reached texels the row is zero exactly where texel_size is 0 (a 1 x 1 texture: all zeros) —; and where any of the
 * eight results is not finite.  No atomic beyond the rasteriser's atomicMin: the same bits from run to run and between ZDR_ACCEL_BRUTE
 * and ZDR_ACCEL_BVH.
 *
 * The call writes BOTH buffers: aovs by the three launches of zdr_scene_texel_aovs (the same launcher, the same bits), then a fourth
 * launch reads the keys those left in `workspace` (zdr_texel_aovs_workspace_bytes) and the normals in aovs.  The raster runs once.  It
 * only enqueues on `stream`, never allocates, never synchronises, and can be captured in a HIP graph without a call before.
 * Errors as for zdr_scene_texel_aovs; in addition ZDR_E_INVALID: a null or misaligned (16 bytes) tangents, any overlap among aovs,
 * tangents and the workspace.  ZDR_E_UNSUPPORTED: a library linked without these kernels (zdr_tangent.hip). */
int zdr_scene_texel_tangents(zdr_scene *scene, int32_t material, int32_t tex_h, int32_t tex_w,
                             float *aovs /* DEVICE tex_h x tex_w x 16 */, float *tangents /* DEVICE tex_h x tex_w x 8 */,
                             void *workspace /* zdr_texel_aovs_workspace_bytes */, void *stream);

/* Texture-space lighting: whether any light reaches a texel, where zdr_scene_texel_aovs says where the texel is.  Per texel, the direct
 * irradiance on the normal's side and the open fraction of the hemisphere (sky visibility; with a finite max_distance, ambient
 * occlusion) — a baker's lightmap, and for texture recovery the mask "lit by nothing".
 *
 * Input.  texel_aovs (DEVICE, tex_h x tex_w x 16) has the layout of zdr_scene_texel_aovs.  Only floats 4..6 (normal n), 8..10 (position p)
 * and 12 (reach) are read: any buffer with those channels is a valid set of surface points.  n is used as it is (not normalised again).
 * Output.  out (DEVICE, tex_h x tex_w x 4, the shape of a material, so zdr_denoise filters it with the same guides):
 *   floats 0..2        irradiance         direct irradiance arriving on the side n points to, per colour channel
 *   float 3            openness           fraction of the cosine-weighted hemisphere about n that is free up to max_distance, in [0, 1]
 * A texel whose reach is not 1, or whose p or n holds a NaN, is four zeros.
 * Draws.  For texel (x, y) and sample s the sampler is the render kernels': sampler_make(cfg, x, y, perm_seed, s) with perm_seed =
 * xxhash32_4(x, y, seed, 0) for CMJ and 0 for pmj02bn.  Four draws, always all four, always in this order: u_ao = next2, u_pick = next,
 * u_prim = next, u_pt = next2 — floats 0..5 of zdr_sampler_dump with nvert = 1.  The light sampler gets u_prim and u_pt handed over, so
 * its environment branch uses u_pt and ignores u_prim: the sequence does not depend on the branch.
 * Irradiance of one sample.  L = sample_light(p, u_pick, u_prim, u_pt) over the scene's current lights (zdr_scene_update_lights,
 * zdr_scene_set_emission_values) and, if one is set, the environment map, which counts as a light exactly as in the render kernels;
 * c = dot(n, L.wi).  If c > 0, L.eval has a positive component and the segment from p towards L.wi over (1e-4, L.dist) is free (the shadow
 * ray of the direct integrator), the sample adds L.eval * (c / max(L.pdf, 1e-4)).  A contribution that holds a NaN or an infinity is dropped.
 * Every primitive can occlude the segment: the brute-force accelerator's mask of primitives that no shadow segment FROM THE SCENE'S OWN
 * SURFACES can meet is not applied, since p is the caller's and may lie anywhere.
 * Openness of one sample.  The direction is to_world(make_onb(n), (r cos phi, r sin phi, sqrt(1 - u_ao.x))), r = sqrt(u_ao.x),
 * phi = 2 pi u_ao.y — the cosine lobe of the BSDF sampler.  The sample adds 1 unless ANY primitive of the scene meets the ray over
 * (1e-4, max_distance): every primitive counts, also those a shadow segment can never meet.  A direction of NaNs hits nothing.
 * Sample range.  irradiance = (1 / spp) x the sum over s in [sample_begin, sample_end), a subrange of [0, spp); openness = the count of
 * open samples of that range / spp, correctly rounded.  The outputs of disjoint ranges add up to the whole: progressive accumulation.
 * Determinism.  The same bits from run to run: no float atomic; the any-hit walks are per lane; where several lanes share a texel's
 * samples (lane j of 2^k takes s = begin + j, begin + j + 2^k, ...; k depends on tex_h x tex_w and the length of the range only) each
 * adds its samples in order and the lanes' sums are added in lane order.  Nothing depends on the launch grid.
 * Gradient.  Of the irradiance, in the lights' emissions and in the environment map: zdr_scene_texel_lighting_backward below.  None in
 * position, normal or geometry, and none of the openness.
 *
 * The caller provides `workspace`, zdr_texel_lighting_workspace_bytes(tex_h, tex_w) bytes (0 = invalid size): a counter and the list of
 * texels to shade.  Three launches on `stream` — clear the counter, compact, shade — that never allocate and never synchronise, with a
 * grid that does not depend on the list's length, so the call can be captured in a HIP graph without a call before.  The scene is only read.
 * ZDR_E_INVALID: a null or misaligned (16 bytes) pointer, struct_size other than sizeof(zdr_texel_lighting_params), a size <= 0, spp = 0,
 * a sample range that is empty or not within [0, spp), max_distance that is not positive, an unknown sampler, spp beyond the pmj02bn
 * tables, an output that overlaps the workspace or the input, a workspace that overlaps the input.  ZDR_E_UNSUPPORTED: more than 2^26
 * texels; pmj02bn without tables; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_lighting_params) */
    int32_t tex_h, tex_w;
    uint32_t spp, sample_begin, sample_end;
    uint32_t seed;
    int32_t sampler;                   /* ZDR_SAMPLER_* */
    float max_distance;                /* > 0; 1e30 = unbounded (sky visibility) */
} zdr_texel_lighting_params;
size_t zdr_texel_lighting_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_scene_texel_lighting(zdr_scene *scene, const zdr_texel_lighting_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                             float *out /* DEVICE tex_h x tex_w x 4 */, void *workspace, void *stream);

/* The adjoint of zdr_scene_texel_lighting's irradiance in the per-model emissions and in the environment map.  With the light list, the
 * sampling tables and visibility held fixed — as zdr_render_backward_emission and zdr_render_backward_env hold them — the forward is
 * exactly linear in both, and this is the transpose of that sparse linear map, with no approximation.
 *
 * Forward, for reference: for texel t and sample s, L = sample_light(p, u_pick, u_prim, u_pt), c = n . L.wi, w = c * rcp(max(L.pdf, 1e-4)).
 * The sample is ACCEPTED iff s lies in the sample range, c > 0, L.eval has a positive component, the shadow segment (1e-4, L.dist) is free
 * and L.eval * w is finite; irradiance[t] = (sum over the accepted samples of L.eval * w) * inv_spp.
 * Adjoint.  With the cotangent d_out (DEVICE, tex_h x tex_w x 4) every accepted sample of a shaded texel t forms
 * term[ch] = (d_out[t][ch] * inv_spp) * w, ch = r, g, b.
 *   Mesh light.  The sample came from the front of mesh light l (the list index sample_light hands out, cos_light > 1e-4):
 *   d_emission[light_insts[l]][ch] += term[ch].
 *   Environment map.  The sample came from the map at uv: d_env[y][x][ch] += k * term[ch] on the four taps of the map's bilinear lookup,
 *   k = (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy.  Taps that the clamp puts on one texel receive both weights.  The alpha channel
 *   is never touched.
 * Both targets are ADDED INTO, as zdr_render_backward does: rows of models that are not lights keep their bits, and so do texels of the
 * map that no sample reads.  d_out[..][3] (the openness' cotangent) is ignored.  The cotangent of a texel that is not shaded (reach != 1,
 * a NaN in position or normal) is never read.  params is the forward's: max_distance plays no part, and the SAME seed is used (no
 * seed + 1 as for zdr_render_backward).  The acceptance test is replayed with the values the scene holds: the emissions and the map must
 * be those of the forward.
 * Held fixed: which models emit, the alias tables and pdfs, visibility and the acceptance test itself.  For one seed the gradient is the
 * exact derivative as long as no accepted light becomes dark in every component.
 * Not promised: bit-stability.  The list of shaded texels varies in order from run to run and the sums use float atomics, so two runs
 * may differ in the last bits.  (The forward's bits stay what they are.)
 *
 * d_emission (DEVICE, ninst x 3) and d_env (DEVICE, the map's h x w x 4) may each be NULL, not both; both in one call are allowed.
 * workspace: zdr_texel_lighting_backward_workspace_bytes(scene, tex_h, tex_w) bytes (0 = invalid) — it takes the handle because the
 * emission accumulator in it depends on the scene's current light count.  Four launches on `stream` — clear, compact, the adjoint of the
 * shading kernel, the gather of the accumulator into d_emission — that never allocate and never synchronise: the call can be captured
 * without a call before.  The scene is only read.
 * Errors as zdr_scene_texel_lighting's (max_distance is not looked at), and ZDR_E_INVALID for: both targets NULL; d_env on a scene
 * without a map; a workspace that overlaps an input or a target, targets that overlap the inputs or each other.  d_emission on a scene
 * without lights is accepted and adds nothing. */
size_t zdr_texel_lighting_backward_workspace_bytes(zdr_scene *scene, int32_t tex_h, int32_t tex_w);   /* 0 = invalid */
int zdr_scene_texel_lighting_backward(zdr_scene *scene, const zdr_texel_lighting_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                                      const float *d_out /* DEVICE tex_h x tex_w x 4 */, float *d_emission /* DEVICE ninst x 3 or NULL */,
                                      float *d_env /* DEVICE map h x w x 4 or NULL */, void *workspace, void *stream);

/* Bounced light: the irradiance that reaches a texel after at least one bounce, and the share of its hemisphere that can bounce light at
 * all — a Lambertian random walk of `bounces` = K vertices from every texel.  albedo / pi x (zdr_scene_texel_lighting's irradiance + this
 * irradiance) is the Lambertian radiosity of the texel.  The irradiance has an adjoint in the materials and the emissions,
 * zdr_scene_texel_bounce_backward below, and one in the environment map, zdr_scene_texel_bounce_backward_env; `surface` has no gradient.
 *
 * Inputs.  texel_aovs (DEVICE, tex_h x tex_w x 16) has the layout of zdr_scene_texel_aovs; floats 4..6 (normal n), 8..10 (position p) and
 * 12 (reach) are read.  A texel is shaded iff reach == 1 and neither n nor p holds a NaN; every other texel is four zeros.  The materials
 * are a packed buffer with dims and nmat as zdr_render_aovs takes them; the slot table is the one the scene holds
 * (zdr_scene_set_material_slots).  ALL materials are read, at the bounce vertices.  The lights are the scene's current ones, the
 * environment map included.
 * Draws.  For texel (x, y) and sample s the sampler state is the baker's: sampler_make(cfg, x, y, perm_seed, s) with perm_seed =
 * xxhash32_4(x, y, seed, 0) for CMJ and 0 for pmj02bn.  u_ao = next2 comes first — the very openness direction of zdr_scene_texel_lighting
 * for the same seed.  Vertex k = 1 .. K then draws u_pick = next, u_prim = next, u_pt = next2, u_lobe = next, u_dir = next2; u_lobe is
 * drawn and ignored.  These are floats 2 + 7 (k - 1) .. of zdr_sampler_dump with nvert = K and rr_depth >= K.  The last vertex draws
 * neither u_lobe nor u_dir.  There is no Russian roulette; 1 <= bounces <= 8.
 * Walk of one sample.  beta = (1, 1, 1), dir = to_world(make_onb(n), lobe(u_ao)) with lobe(u) = (r cos phi, r sin phi, sqrt(1 - u.x)),
 * r = sqrt(u.x), phi = 2 pi u.y.  The first segment leaves p over (1e-4, 1e30): the openness ray.  Later segments leave
 * offset_ray_origin(p_k, ng_k) over (0, 1e30), as the direct integrator sends its BSDF ray.  For k = 1 .. K:
 *   1. a NaN in dir ends the walk;
 *   2. h = the closest hit of the segment; a miss ends the walk.  Light that a segment sees directly, the environment included, is the
 *      previous vertex's direct light and is counted by the light samples only;
 *   3. it = surface_interact(h); the walk ends if dot(-dir, it.ng) < 1e-4 or dot(-dir, it.ns) < 1e-4 (the integrators' one-sidedness);
 *   4. the walk ends if the model has no material (slot < 0: a light or a blocker);
 *   5. if k = 1 the sample counts for `surface`;
 *   6. beta *= read_bsdf(material of the slot, it.uv).rgb.  Roughness is ignored: with cosine sampling a Lambertian bounce's
 *      f cos / pdf is the albedo, so no pi appears anywhere;
 *   7. one light sample: L = sample_light(it.p, u_pick, u_prim, u_pt), c = it.ns . L.wi.  It is accepted iff c > 0, L.eval has a positive
 *      component, the segment from it.p towards L.wi over (1e-4, L.dist) is free and add = (beta * L.eval) * (c * rcp(max(L.pdf, 1e-4)))
 *      is finite.  An accepted sample gives E += add;
 *   8. dir = to_world(make_onb(it.ns), lobe(u_dir)); the walk ends if dot(dir, it.ng) < 1e-4 or the lobe's z is below 1e-4.
 * Vertex k's add does not depend on K (prefix property).
 * Output.  out (DEVICE, tex_h x tex_w x 4):
 *   floats 0..2        irradiance         (sum over s of E_s) / spp: the irradiance arriving after 1 .. K bounces
 *   float 3            surface            first segments that landed on the front of a model with a material, over spp
 * Sample range.  [sample_begin, sample_end) is a subrange of [0, spp), and the outputs of disjoint ranges add up.
 * Determinism.  Lanes per texel follow the rule of zdr_scene_texel_lighting — 2^k lanes, k = zdr_texel_bounce_lanes_shift(tex_h, tex_w,
 * sample_begin, sample_end), from the texture's size and the length of the range alone; lane j takes s = begin + j, begin + j + 2^k, ... —
 * and a lane adds every accepted add into one accumulator, s ascending and, within s, k ascending.  Lane 0 of a texel then adds the lanes'
 * sums in lane order and multiplies by 1 / spp (IEEE division); surface is a count divided by spp, correctly rounded.  The same bits
 * from run to run, whatever the grid and the order of the list: no float atomic, and the walks are per lane.
 * Limits.  Lambertian bounces only — GGX is ignored, so on glossy materials this is not zdr_render_forward's radiance.  K truncates: the
 * result is biased low by the bounces beyond it.  With the same seed the walk shares u_ao with the openness ray, and vertex 1 shares
 * its light draws with zdr_scene_texel_lighting's own sample: either output is unbiased, but the two are correlated.
 *
 * workspace: zdr_texel_bounce_workspace_bytes(tex_h, tex_w) bytes (0 = invalid size): a counter and the list of texels to shade.  Three
 * launches on `stream` — clear the counter, compact (one returning atomic per workgroup), shade — that never allocate and never
 * synchronise; the material table travels as a kernel argument, so the call can be captured in a HIP graph without a call before (on a
 * scene whose slot table has been set: a table that was never set would have to be created, which a capture refuses).
 * ZDR_E_INVALID: a null or misaligned (16 bytes) pointer, struct_size other than sizeof(zdr_texel_bounce_params), a size <= 0, spp = 0,
 * a sample range that is empty or not within [0, spp), bounces outside [1, 8], nmat outside [1, ZDR_MAX_MATERIALS], a slot beyond nmat,
 * an unknown sampler, an output that overlaps the workspace or an input, a workspace that overlaps an input.  ZDR_E_UNSUPPORTED: more
 * than 2^26 texels; pmj02bn without tables; a library linked without these kernels (zdr_bounce.hip).
 *
 * zdr_texel_bounce_dump serves the tests, in the tradition of zdr_path_dump: queries (DEVICE, n x 3 int32 {x, y, s}), one lane per query,
 * the same walk with a recorder.  A row of out is 4 + 12 K floats: the header {bits(nvert), surface, 0, 0}, then per vertex
 * {bits(inst), bits(prim), u, v, bits(flags), beta.rgb after the vertex, add.rgb, 0} — instance, input triangle and barycentrics as
 * zdr_trace_closest reports a hit.  Flag bits: 0 shaded (front and has a material), 1 the light sample is lit (c > 0 and eval positive),
 * 2 the shadow segment is free, 3 add accepted, 4 the walk goes on to a next vertex (never set at vertex K).  A vertex where the walk
 * ends is recorded with its flags; nvert counts the recorded vertices (the segments that hit).  A query outside the texture or the
 * sample range, or of a texel that is not shaded, is a row of zeros. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_bounce_params) */
    int32_t tex_h, tex_w;
    uint32_t spp;
    uint32_t seed;
    int32_t sampler;                   /* ZDR_SAMPLER_* */
    uint32_t sample_begin, sample_end;
    int32_t bounces;                   /* K, 1 .. 8 */
} zdr_texel_bounce_params;
size_t zdr_texel_bounce_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_texel_bounce_lanes_shift(int32_t tex_h, int32_t tex_w, uint32_t sample_begin, uint32_t sample_end);   /* k of 2^k lanes per texel; -1 = invalid */
int zdr_scene_texel_bounce(zdr_scene *scene, const zdr_texel_bounce_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                           const float *materials /* DEVICE packed */, const int32_t *dims /* HOST nmat x {h, w} */, uint32_t nmat,
                           float *out /* DEVICE tex_h x tex_w x 4 */, void *workspace, void *stream);
int zdr_texel_bounce_dump(zdr_scene *scene, const zdr_texel_bounce_params *params, const float *texel_aovs, const float *materials,
                          const int32_t *dims, uint32_t nmat, const int32_t *queries /* DEVICE n x 3 */, uint32_t n,
                          float *out /* DEVICE n x (4 + 12 bounces) */, void *stream);

/* The adjoint of zdr_scene_texel_bounce's irradiance: the gradient in the rgb of the material texels and in the lights' emissions.  The
 * walk's directions come from cosine lobes about the normals, so neither the hits nor the draws depend on the materials: for one seed the
 * bake is a polynomial in the material texels, of degree <= bounces per channel and exactly linear for bounces = 1, and exactly linear
 * in the emissions.  Both gradients are exact transposes, not approximations.
 *
 * Definition.  Consider one shaded texel t and one sample s of the range.  The walk of zdr_scene_texel_bounce visits shaded vertices
 * k = 1 .. n, n <= bounces.  Vertex k has the albedo a_k (rgb) = read_bsdf(material of the vertex's slot, it.uv).rgb, beta_k = the product
 * of a_i over i <= k with beta_0 = 1, the weight w_k = L.eval x c x rcp(max(L.pdf, 1e-4)) and the forward's acceptance bit A_k (step 7 of
 * the walk, with the forward's beta).  The forward is out[t].rgb = inv_spp x sum over s and k of A_k beta_k w_k.  With the cotangent
 * gamma = d_out[t].rgb x inv_spp, all per channel:
 *     Q_{n+1} = 0,   Q_k = A_k w_k + a_{k+1} Q_{k+1}
 *     d a_k   = gamma x beta_{k-1} x Q_k
 * Materials.  d a_k goes to the four taps of the bilinear lookup of vertex k, in the material of the vertex's slot, with the weights of
 * read_bsdf; taps that the clamp puts on one texel receive both weights.  Only rgb is written: the roughness channel is never touched.
 * The rule is division free: the gradient is correct where an albedo component is 0, and an all-black material still receives the
 * gradient of its first vertex.  A term that is not finite is dropped, as the forward drops a non-finite add.
 * Emissions.  An accepted vertex whose sample came from the front of mesh light l adds gamma x beta_k x c x rcp(max(L.pdf, 1e-4)) to
 * d_emission[light_insts[l]]: the rule of zdr_scene_texel_lighting_backward with beta_k in front.
 * Both targets are ADDED INTO: texels that no vertex reads keep their bits, and so do the rows of models that are not lights.
 * d_out[..., 3], the cotangent of `surface`, is ignored; the cotangent of a texel that is not shaded is never read.  The seed is the
 * forward's own, and the scene must hold the forward's emissions and map.
 * Held fixed: the walks, the light list, the sampling tables, visibility and the acceptance bits.
 * Not differentiated: the geometry, the GGX lobe (which the forward ignores too).  The environment map through the bounce has a call of
 * its own, zdr_scene_texel_bounce_backward_env below.
 * Not promised: bit-stability.  The list of shaded texels varies in order from run to run and the sums use float atomics, so two runs
 * may differ in the last bits.  (The forward's bits stay what they are.)
 * Operation order.  Lanes, trips and draws are the forward's (zdr_texel_bounce_lanes_shift).  Per trip a lane (1) replays the walk and
 * records per vertex {uv, slot, A_k w_k, a_k} — A_k is decided on add = (beta_k * L.eval) * (c * rcp(max(L.pdf, 1e-4))) as in the forward;
 * the emission term (gamma * beta_k) * (c * rcp(...)) is added here —, (2) forms Q_k = A_k w_k + a_{k+1} * Q_{k+1} from the last vertex
 * to the first, (3) forms d a_k = (gamma * beta_{k-1}) * Q_k from the first vertex to the last, with beta_0 = 1 and beta_k = beta_{k-1} *
 * a_k, and hands each to the gradient scatter of the material-table backward calls: k_m * d a_k added to tap m's staging cell, the cells
 * and their copies summed per texel (in float64 where a material has copies), then added to d_materials.
 *
 * d_materials (DEVICE, packed like materials) and d_emission (DEVICE, ninst x 3) may each be NULL, not both.
 * workspace: zdr_texel_bounce_backward_workspace_bytes(scene, tex_h, tex_w, dims, nmat) bytes (0 = invalid) — the handle because the
 * emission accumulator depends on the scene's current light count, the material dims because the staging cells and their copies (those
 * of every material-table backward call: a 1 x 1 material is replicated, not an atomic hot spot) depend on them.  It needs no
 * initialisation.  Up to five launches on `stream` — clear (a kernel), compact, the adjoint of the shading kernel, the gather of the
 * cells into d_materials, the gather of the accumulator into d_emission — that never allocate and never synchronise: the call can be
 * captured without a call before, as the forward.
 * Errors as zdr_scene_texel_bounce's, and ZDR_E_INVALID for: both targets NULL; a misaligned target (d_materials 16 bytes, d_emission 4);
 * a workspace that overlaps an input or a target, targets that overlap the inputs or each other.  ZDR_E_UNSUPPORTED: a library linked
 * without these kernels (zdr_bouncegrad.hip).  d_emission on a scene without lights is accepted and adds nothing. */
size_t zdr_texel_bounce_backward_workspace_bytes(zdr_scene *scene, int32_t tex_h, int32_t tex_w, const int32_t *dims /* HOST nmat x {h, w} */,
                                                 uint32_t nmat);   /* 0 = invalid */
int zdr_scene_texel_bounce_backward(zdr_scene *scene, const zdr_texel_bounce_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                                    const float *d_out /* DEVICE tex_h x tex_w x 4 */, const float *materials /* DEVICE packed */,
                                    const int32_t *dims /* HOST nmat x {h, w} */, uint32_t nmat,
                                    float *d_materials /* DEVICE packed like materials, +=, or NULL */,
                                    float *d_emission /* DEVICE ninst x 3, +=, or NULL */, void *workspace, void *stream);

/* The adjoint of zdr_scene_texel_bounce's irradiance in the environment map.  The forward reads the map at every bounce vertex whose light
 * sample falls on it, and the bake is exactly linear in the map's texels: this is the transpose of that sparse linear map, with no
 * approximation.
 *
 * Held fixed: everything zdr_scene_texel_bounce_backward holds fixed — the walks, the light list, the sampling tables, visibility and the
 * acceptance bits.
 * Definition.  Consider one shaded texel t and one sample s of the range.  Vertex k of the forward's walk has beta_k (the forward's, the
 * materials included), ws = c * rcp(max(L.pdf, 1e-4)) and the forward's acceptance bit A_k, decided on add = (beta_k * L.eval) * ws as in
 * the forward.  With gamma = d_out[t].rgb * inv_spp, an accepted vertex whose light sample came from the environment map at uv (the
 * env_uv of sample_light: uv.x >= 0) forms
 *     term[ch] = (gamma[ch] * beta_k[ch]) * ws,   ch = r, g, b
 * and d_env[y][x][ch] += k_m * term[ch] on the four taps of the map's bilinear lookup (env_lookup), k_m = (1 - fx)(1 - fy), fx (1 - fy),
 * (1 - fx) fy, fx fy.  Taps that the clamp puts on one texel receive both weights.  This is zdr_scene_texel_lighting_backward's rule with
 * beta_k in front.  A term that is not finite is dropped.  The alpha channel is never touched.
 * d_env is ADDED INTO: texels of the map that no sample reads keep their bits.  d_out[..., 3], the cotangent of `surface`, is ignored; the
 * cotangent of a texel that is not shaded is never read.  The seed is the forward's own, and the scene must hold the forward's emissions
 * and map: the acceptance test is replayed with them.
 * Not promised: bit-stability.  The list of shaded texels varies in order from run to run and the sums use float atomics, so two runs
 * may differ in the last bits.  (The forward's bits stay what they are.)
 * Operation order.  Lanes, trips and draws are the forward's (zdr_texel_bounce_lanes_shift); a lane replays the walk vertex by vertex and
 * carries beta_k.  Per vertex index the accepted environment samples of a wave are merged by map cell — the merge of
 * zdr_scene_texel_lighting_backward: up to four cells per vertex index are summed on chip and added as 12 floats each, the samples of
 * further cells add their 12 floats one by one.  This is a replay of its own: a caller who wants the materials' or the emissions'
 * gradient too calls zdr_scene_texel_bounce_backward as well.
 *
 * workspace: zdr_texel_bounce_backward_env_workspace_bytes(tex_h, tex_w) bytes (0 = invalid size): a header — word 0 the shaded texels,
 * word 1 the accepted environment samples, word 2 the groups of 12 floats that went to memory after the merge — and the list of texels.
 * It needs no initialisation.  Three launches on `stream` — clear (a kernel), compact, the replay — that never allocate and never
 * synchronise: the call can be captured without a call before, as the forward.
 * Errors as zdr_scene_texel_bounce_backward's, and ZDR_E_INVALID for: a NULL or misaligned (16 bytes) d_env; a d_env that overlaps an
 * input or the workspace; a scene without an environment map ("d_env given, but the scene has no environment map", as
 * zdr_render_backward_env).  ZDR_E_UNSUPPORTED: a library linked without these kernels (zdr_bounceenv.hip). */
size_t zdr_texel_bounce_backward_env_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_scene_texel_bounce_backward_env(zdr_scene *scene, const zdr_texel_bounce_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                                        const float *d_out /* DEVICE tex_h x tex_w x 4 */, const float *materials /* DEVICE packed */,
                                        const int32_t *dims /* HOST nmat x {h, w} */, uint32_t nmat,
                                        float *d_env /* DEVICE map h x w x 4, += */, void *workspace, void *stream);

/* Push-pull: fills the texels of a texture that a weight marks as unknown from the ones it marks as known, through a weighted pyramid — a
 * baker's seam padding — and the adjoint of that map with respect to the texture.  No scene handle.  The known texels come out bit for
 * bit as they went in; with the weights held fixed the map is linear in the texture, so y = K x is also a reparameterisation of a
 * material whose holes are always the smooth continuation of their chart, and d_x = K^T g carries the gradient that lands on a hole back
 * to the known texels that determine it.
 *
 * Inputs: a texture x (H, W, 4) and a weight w (H, W), such as the coverage of zdr_scene_texel_aovs.  The output y has the shape of x.
 * Level sizes.  (H_0, W_0) = (H, W);  (H_{l+1}, W_{l+1}) = (ceil(H_l / 2), ceil(W_l / 2));  L is the first level of size 1 x 1, and
 * min(that, levels) if levels > 0.
 * Level 0.  a_0 = w clamped to [0, 1], NaN -> 0;  p_0 = a_0 x where a_0 > 0, else 0.  A texel of weight 0 is never read into the result,
 * whatever it holds, NaN and infinity included.
 * Push, l = 0 .. L - 1.  The children of (i, j) are (2i + {0, 1}, 2j + {0, 1}); children outside the level count as 0.
 *   S = (a_00 + a_01) + (a_10 + a_11),  P = (p_00 + p_01) + (p_10 + p_11),
 *   a_{l+1} = min(S, 1),  r_{l+1} = a_{l+1} / S where S > 0, else 0,  p_{l+1} = P r_{l+1}.
 * Top.  y_L = p_L / a_L where a_L > 0, else 0.
 * Pull, l = L - 1 .. 0.  y_l = p_l + (1 - a_l) U(y_{l+1});  at level 0, y = x (the same bits, by selection) where a_0 = 1.
 * Upsampling.  U is bilinear from the coarser level, applied separably: for fine index i of an axis, c = i >> 1 and nb = c + 1 if i is
 * odd, else c - 1, clamped to the coarser level; the value is 0.75 v[c] + 0.25 v[nb].  Along the row (x) first, then across rows.
 * It follows that every output texel is a convex combination of the inputs whose weight is positive, that a texture which is constant
 * where w > 0 comes out constant everywhere, that w = 1 everywhere gives y = x bit for bit and w = 0 everywhere gives y = 0.  Holes that
 * a pyramid cut short by `levels` cannot reach are 0.
 * Adjoint, d_x = K^T g for the same w:  G_0 = g;  G_{l+1} = U^T((1 - a_l) G_l);  q_L = G_L / a_L where a_L > 0, else 0;
 * q_l = G_l + r_{l+1}[parent] q_{l+1}[parent];  d_x = a_0 q_0 (0 where a_0 = 0).  U^T is a gather: a coarse index c collects from the fine
 * indices 2c - 1 .. 2c + 2 of each axis, the taps a clamped border folds onto it included; no atomic is needed.  The adjoint rebuilds
 * a_l and r_l from w itself: it needs nothing that a forward call left behind.  The WEIGHTS receive NO gradient: they are held fixed.
 * The kernels are compiled without contraction, so the result is defined by the operation order above.
 *
 * All pointers are DEVICE pointers, 16-byte aligned; weight is H x W, x / out / d_out / d_x are H x W x 4.  The caller provides
 * `workspace`, at least zdr_push_pull_workspace_bytes(params) bytes (0 = invalid params; never 0 otherwise): the levels >= 1.  Both
 * calls only enqueue on `stream`: they never allocate and never synchronise, so they can be captured in a HIP graph without a call
 * before.  No float atomic: the same bits from run to run, whatever the workspace held; one workspace may serve both calls, one call in
 * flight at a time.  out and d_x are overwritten and must not overlap an input or the workspace.
 * ZDR_E_INVALID: struct_size other than sizeof(zdr_push_pull_params), a width or height <= 0, levels < 0, a null or misaligned pointer,
 * an output that overlaps an input or the workspace, a workspace that overlaps an input (byte ranges as the parameters size them).
 * ZDR_E_UNSUPPORTED: more than 2^26 texels, the cap of zdr_scene_texel_aovs; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_push_pull_params) */
    int32_t width, height, levels;     /* levels: 0 = down to 1 x 1 */
} zdr_push_pull_params;
size_t zdr_push_pull_workspace_bytes(const zdr_push_pull_params *params);   /* 0 = invalid */
int zdr_push_pull(const zdr_push_pull_params *params, const float *weight, const float *x, float *out, void *workspace, void *stream);
int zdr_push_pull_backward(const zdr_push_pull_params *params, const float *weight, const float *d_out, float *d_x, void *workspace,
                           void *stream);

/* Texture-space views (projective texturing): what a camera sees of each texel, the photograph it took gathered into texture space, and
 * the adjoint of that gather.  Two halves, split where the cost and the differentiability split.
 *
 * 1. zdr_scene_texel_view: geometry.  Needs the scene, costs one any-hit ray per texel, carries no gradient.
 * texel_aovs: a tex_h x tex_w x 16 buffer in the layout of zdr_scene_texel_aovs, of which only the normal (floats 4..6), texel_size (7),
 * the position (8..10) and reach (12) are read — any set of surface points is valid input, as for zdr_scene_texel_lighting.  A texel is
 * SHADED iff reach == 1 and neither its normal nor its position holds a NaN; every other texel gets eight zeros.  The camera's frame
 * o, fwd, right, upp, tan = tan(fov / 2), aspect = height / width is the one a render with `camera`, `width` and `height` uses.
 * With v = p - o, z = v . fwd, dist = |v|, a shaded texel gets
 *   float 0     visible    1 iff z > 0 (in front), 0 <= X < width and 0 <= Y < height (inside) and the segment to the camera is free, else 0
 *   float 1     cosine     n . wi, wi = (o - p) / dist, signed.  A weight, not a test: the renderer has no facing test, `visible` has none
 *   floats 2, 3 pixel      X = ((v . right) / z / tan + 1) width / 2,  Y = (-(v . upp) / z / (tan aspect) + 1) height / 2: the exact inverse
 *                          of the camera ray with the pixel jitter as the fractional part; pixel x covers [x, x + 1).  0 when z <= 0
 *   floats 4, 5 depth, distance   z and dist
 *   float 6     scale      on-screen length of one texel in pixels, texel_size (width / 2) / (tan z); 0 when z <= 0.
 *                          scale^2 |cosine| approximates the texel's area in pixels
 *   float 7                0
 * The segment starts at p with direction wi and the interval (1e-4, dist); it is tested against every primitive (the any-hit query of
 * zdr_trace_any), and only for texels in front and inside.  Products and sums are float32 in the order written (dot products from x to
 * z), divisions and the square root IEEE, nothing contracted.  No float atomic and no dependence on the order of the work: the same bits
 * from run to run.  `workspace`: at least zdr_texel_view_workspace_bytes(tex_h, tex_w) bytes (0 = invalid size), contents irrelevant.
 * The call only enqueues on `stream`; it never allocates and never synchronises, and can be captured in a HIP graph without a call
 * before.
 * ZDR_E_INVALID: a null or misaligned (16 bytes) pointer, struct_size other than sizeof(zdr_texel_view_params), a size <= 0, a fov that
 * is not finite or not in (0, pi), an output that overlaps the workspace or the input, a workspace that overlaps the input.
 * ZDR_E_UNSUPPORTED: more than 2^26 texels or 2^28 pixels; a library linked without these kernels.
 *
 * 2. zdr_texel_gather, zdr_texel_gather_backward: the gather and its adjoint.  No scene handle, no workspace.
 * view: a tex_h x tex_w x 8 view buffer, of which only floats 0 (visible), 2 and 3 (X, Y) are read; image: height x width x 4.
 * Forward, color (tex_h x tex_w x 4, overwritten).  Where visible is 0 (or NaN) the colour is 0 and the image is NOT read: what lies
 * behind an invisible texel, NaN included, never reaches the result, and X, Y may hold anything there.  Otherwise, in this order:
 *   fx = X - 0.5, fy = Y - 0.5;  x0 = floor(fx), y0 = floor(fy);  tx = fx - x0, ty = fy - y0;
 *   taps x0 and x0 + 1 clamped to [0, width - 1], y0 and y0 + 1 clamped to [0, height - 1] (the weights come from the unclamped fraction);
 *   top = c(y0, x0) + (c(y0, x1) - c(y0, x0)) tx,  bot = c(y1, x0) + (c(y1, x1) - c(y1, x0)) tx,  color = visible (top + (bot - top) ty)
 * per channel, uncontracted: X, Y at a pixel's centre return that pixel bit for bit, and a 1 x 1 image returns its pixel.  The gather
 * POINT-SAMPLES: a texel that covers many pixels (scale >> 1) aliases; zdr_texel_gather_mip below ("Prefiltered gather") is the remedy.
 * Adjoint, d_image (height x width x 4) ADDED INTO — the caller zeroes it: for the same four taps
 *   d_image[tap] += (w visible) d_color,  w = (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty,
 * one float atomic per tap and channel.  With the view held fixed the map is linear in the image and this is its transpose, up to the
 * rounding of the four products and the order of the additions (which varies from run to run).  The VIEW BUFFER receives NO gradient.
 * Both calls only enqueue on `stream` and can be captured without a call before.
 * ZDR_E_INVALID: struct_size other than sizeof(zdr_texel_gather_params), a size <= 0, a null or misaligned (16 bytes) pointer, an output
 * that overlaps an input.  ZDR_E_UNSUPPORTED: more than 2^26 texels or 2^28 pixels; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_view_params) */
    int32_t tex_h, tex_w;
    int32_t width, height;             /* of the camera's image */
    zdr_camera camera;
} zdr_texel_view_params;
size_t zdr_texel_view_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_scene_texel_view(zdr_scene *scene, const zdr_texel_view_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                         float *out /* DEVICE tex_h x tex_w x 8 */, void *workspace, void *stream);
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_gather_params) */
    int32_t tex_h, tex_w;
    int32_t width, height;             /* of the image */
} zdr_texel_gather_params;
int zdr_texel_gather(const zdr_texel_gather_params *params, const float *view, const float *image, float *color, void *stream);
int zdr_texel_gather_backward(const zdr_texel_gather_params *params, const float *view, const float *d_color, float *d_image, void *stream);

/* Prefiltered gather: a mip pyramid of the image, a trilinear gather that takes the level from each texel's on-screen footprint (float 6
 * of the view buffer, scale), and the exact transposes of both, so that a gradient reaches every pixel under a texel's footprint.  No
 * scene handle.
 *
 * Pyramid.  Level 0 is the image, height x width x 4.  (w_{l+1}, h_{l+1}) = (ceil(w_l / 2), ceil(h_l / 2));  L is the first level of size
 * 1 x 1, and min(that, levels) if levels > 0.  The image is thought of as continued by its border pixels: pixel (row i, column j) of
 * level l + 1 is
 *   ((a00 + a01) + (a10 + a11)) * 0.25,   a_rc = level l at (row min(2i + r, h_l - 1), column min(2j + c, w_l - 1)),
 * per channel, uncontracted, in that order.  So for an odd size the last coarse pixel counts the last fine pixel twice and the corner
 * pixel counts it four times, and a constant image has constant levels of the same bits.  The levels >= 1 are packed one after another
 * (level 1 first, rows of float4) into one buffer, the PYRAMID, of zdr_image_pyramid_bytes(params) bytes: 0 = invalid parameters, never 0
 * otherwise (16 when L = 0).  Level 0 is never copied.
 * Pyramid adjoint, zdr_image_pyramid_backward.  d_pyramid holds cotangents G_1 .. G_L in the pyramid's layout.  T_L = G_L;
 *   T_l[y, x] = G_l[y, x] + (0.25 m_l(y, x)) T_{l+1}[y >> 1, x >> 1],   m_l = mx my,
 * mx = 2 if x is the last index of an odd-width level, else 1, my likewise for rows;  d_image[y, x] += (0.25 m_0(y, x)) T_1[y >> 1, x >> 1],
 * ADDED INTO as zdr_texel_gather_backward adds.  A gather (every fine pixel has one parent): no atomic, the same bits from run to run.
 * d_pyramid is a WORKSPACE: its contents after the call are unspecified.
 *
 * Level of a texel.  s = scale * footprint (a float32 product; footprint: finite, > 0, 1 by default; 0.5 sharpens by one level);
 * s = max(s, 1), NaN -> 1;  l0 = the binary exponent of s, taken from its bits;  m = s 2^-l0 in [1, 2);  f = 0 if m == 1 (by selection),
 * else min(log2f(m), 1);  if l0 >= L then l0 = L and f = 0.  The split is exact integer work; only f carries rounding, and the result is
 * continuous in it.
 * Mip gather, zdr_texel_gather_mip: color (tex_h x tex_w x 4, overwritten).  Where visible is 0 or NaN the colour is 0 and neither the
 * image nor the pyramid is read for that texel.  Otherwise lo = the bilinear sample of level l0 at (X 2^-l0, Y 2^-l0) — the scaling is
 * exact — by the tap rule of zdr_texel_gather with that level's width and height, operation for operation.  If f == 0 the upper level is
 * NOT READ and c = lo; otherwise hi is the same sample of level l0 + 1 and c = lo + (hi - lo) f.  color = visible c.
 * It follows that wherever s <= 1 the result is zdr_texel_gather's bit for bit; that where scale is 2^k (k <= L) and footprint is 1 it is,
 * bit for bit, zdr_texel_gather of level k with X, Y scaled by 2^-k; and that a constant image comes out as visible times that constant.
 * Mip gather adjoint, zdr_texel_gather_mip_backward: ADDED INTO d_image (level 0) and d_pyramid (the levels >= 1, the pyramid's layout; the
 * caller zeroes it), one float atomic per tap and channel.  Each lower tap receives ((w (1 - f)) visible) d_color, each upper tap, only
 * where f != 0, ((w f) visible) d_color, w the four bilinear products of zdr_texel_gather_backward; with f == 0 that is the very product
 * zdr_texel_gather_backward adds.  The VIEW BUFFER receives NO gradient.  The full image gradient is this call followed by
 * zdr_image_pyramid_backward on d_pyramid.
 * The filter is ISOTROPIC: scale is the footprint's long axis, so grazing texels (|cosine| << 1) are over-blurred across the short one;
 * anisotropic filtering needs footprint axes that the view buffer does not carry: zdr_texel_footprint and zdr_texel_gather_aniso below.
 *
 * All pointers are DEVICE pointers, 16-byte aligned.  The calls only enqueue on `stream`: they never allocate and never synchronise, and
 * can be captured in a HIP graph without a call before.
 * ZDR_E_INVALID: a wrong struct_size, a size <= 0, levels < 0, a footprint that is not finite or not > 0, a null or misaligned pointer, an
 * output that overlaps an input or another output (byte ranges as the parameters size them).
 * ZDR_E_UNSUPPORTED: more than 2^26 texels or 2^28 pixels; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_image_pyramid_params) */
    int32_t width, height, levels;     /* levels: 0 = down to 1 x 1 */
} zdr_image_pyramid_params;
size_t zdr_image_pyramid_bytes(const zdr_image_pyramid_params *params);   /* 0 = invalid */
int zdr_image_pyramid(const zdr_image_pyramid_params *params, const float *image, float *pyramid, void *stream);
int zdr_image_pyramid_backward(const zdr_image_pyramid_params *params, float *d_pyramid, float *d_image, void *stream);
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_gather_mip_params) */
    int32_t tex_h, tex_w;
    int32_t width, height, levels;     /* of the image; levels as zdr_image_pyramid_params.levels */
    float footprint;
} zdr_texel_gather_mip_params;
int zdr_texel_gather_mip(const zdr_texel_gather_mip_params *params, const float *view, const float *image, const float *pyramid, float *color,
                         void *stream);
int zdr_texel_gather_mip_backward(const zdr_texel_gather_mip_params *params, const float *view, const float *d_color, float *d_image,
                                  float *d_pyramid, void *stream);

/* Anisotropic gather: the on-screen footprint ELLIPSE of every texel, a gather that places up to max_aniso trilinear probes of the mip
 * gather along the ellipse's major axis — the way a texture unit filters anisotropically — and that gather's exact transpose.  The
 * pyramid is zdr_image_pyramid's, unchanged.  No scene handle, no workspace, one launch per call.
 *
 * Footprint buffer, zdr_texel_footprint: out (tex_h x tex_w x 4, overwritten) from the texel buffer of zdr_scene_texel_aovs (normal n,
 * texel_size, position p, reach) and a camera, whose frame (o, fwd, right, upp, tan, aspect, half_w = width / 2, half_h = height / 2) is
 * exactly the one zdr_scene_texel_view derives.  A texel that is not shaded (the view's rule: reach == 1 and no NaN in normal or
 * position), or that has z <= 0, or for which any of the four results is not finite, gets four zeros.  For the others, in float32,
 * uncontracted, divisions and roots IEEE, dot products from x to z:
 *   v = p - o,  z = v.fwd,  a = v.right,  b = v.upp
 *   gX = (right z - fwd a) (half_w / (tan (z z))),   gY = -((upp z - fwd b) (half_h / ((tan aspect) (z z))))
 * — the derivatives of the view buffer's X, Y with respect to the world position —, (t1, t2) = tangent and binormal of the kernels'
 * make_onb(n),
 *   m00 = texel_size (gX.t1), m01 = texel_size (gX.t2), m10 = texel_size (gY.t1), m11 = texel_size (gY.t2)
 *   P = m00^2 + m01^2,  Q = m10^2 + m11^2,  R = m00 m10 + m01 m11,  hd = 0.5 (P - Q),  d = sqrt(hd^2 + R^2)
 *   major = sqrt(0.5 (P + Q) + d),   minor = |m00 m11 - m01 m10| / major, 0 if major == 0
 * (the determinant, not the smaller eigenvalue 0.5 (P + Q) - d, which cancels at grazing angles);  the direction e = (hd + d, R) if
 * P >= Q, else (R, 0.5 (Q - P) + d) — no cancellation in the component that carries the length —, divided by sqrt(e.e), (1, 0) if that
 * is 0.  Floats of a row: 0, 1 = major e (pixels), 2 = minor, 3 = major.  Because M M^T = texel_size^2 J (I - n n^T) J^T, the ellipse
 * does not depend on the tangent basis that make_onb returns.  The texel is taken as a SQUARE PATCH of side texel_size in its tangent
 * plane: that is the default, and it does not model the stretch of the UV mapping itself (a non-square texture, a stretched chart).
 * zdr_texel_footprint_tangents below follows the mapping.  No atomic: the same bits from run to run.
 *
 * Footprint from UV tangents, zdr_texel_footprint_tangents: the same params, the same out, and the tangent buffer of
 * zdr_scene_texel_tangents in addition.  The texel is the PARALLELOGRAM p + a Tx + b Ty, a, b in [-1/2, 1/2]: its true patch.  The shaded
 * rule, the camera frame, z, gX and gY are those above.  A texel whose tangent row is eight zeros gets four zeros.  Otherwise
 *   m00 = gX.Tx,  m01 = gX.Ty,  m10 = gY.Tx,  m11 = gY.Ty
 * — no texel_size, no make_onb — and P, Q, R, hd, d, major, minor, the direction and the finiteness test follow operation for operation
 * (one device function, csrc/footprint.h, called by both kernels).  The output feeds zdr_texel_gather_aniso, its adjoint and
 * zdr_gather_plan_* unchanged: they read a footprint buffer and do not care who wrote it.  With max_aniso = 1 that gather is the mip
 * gather at the texel's TRUE long axis: the remedy for zdr_texel_gather_mip on non-square textures, whose level comes from the view
 * buffer's scale (texel_size).  One launch of zdr_tangent.hip; errors as zdr_texel_footprint, tangents counted among the inputs.
 *
 * Probes of a texel.  A = major * footprint, B = minor * footprint (float32 products; footprint: finite, > 0; max_aniso: 1 .. 16).  If not
 * A > 1 (a NaN too): N = 1, s = 1.  Else B' = max(B, A / max_aniso, 1) (a NaN B is passed over), q = ceil(A / B' - 0.125),
 * N = q if 1 <= q <= max_aniso, max_aniso if q is larger, 1 otherwise (a NaN), s = B'.  The offset of 1/8: a plane parallel to the image
 * plane projects by a similarity, its ratio is exactly 1 in exact arithmetic, and without the offset float32 would make N toggle between
 * 1 and 2 across such a surface.  (l0, f) = the level split of zdr_texel_gather_mip applied to s with that routine's footprint at 1.
 * Anisotropic gather, zdr_texel_gather_aniso: color (tex_h x tex_w x 4, overwritten).  Where visible is 0 or NaN the colour is 0 and
 * NOTHING ELSE is read for that texel: no footprint row, no image, no pyramid.  Otherwise for probe i = 0 .. N - 1
 *   t_i = (2 i + 1 - N) / (2 N)  (both exact as floats, one IEEE division),
 *   X_i = X + (t_i footprint) major_x,   Y_i = Y + (t_i footprint) major_y,
 *   c_i = the trilinear sample of zdr_texel_gather_mip at (X_i, Y_i) with (l0, f), operation for operation (the upper level is not
 *         read where f == 0),
 *   color = visible (((c_0 + c_1) + c_2 ...) (1 / N)),   1 / N one IEEE division.
 * It follows that wherever A <= 1 the result is zdr_texel_gather's bit for bit; that a footprint row (scale, 0, scale, scale), or
 * max_aniso = 1 with major = scale, gives zdr_texel_gather_mip's bits; and that a constant image comes out as visible times that
 * constant up to the rounding of N (1 / N).
 * Adjoint, zdr_texel_gather_aniso_backward: ADDED INTO d_image (level 0) and d_pyramid (the levels >= 1, the pyramid's layout; the
 * caller zeroes it), one float atomic per tap, probe and channel.  Per probe each lower tap receives (((w (1 - f)) (1 / N)) visible)
 * d_color, each upper tap, only where f != 0, (((w f) (1 / N)) visible) d_color, w the four bilinear products of
 * zdr_texel_gather_backward.  The VIEW and FOOTPRINT buffers receive NO gradient.  The full image gradient is this call followed by
 * zdr_image_pyramid_backward on d_pyramid.
 *
 * All pointers are DEVICE pointers, 16-byte aligned.  The calls only enqueue on `stream`: they never allocate and never synchronise, and
 * can be captured in a HIP graph without a call before.
 * ZDR_E_INVALID: a wrong struct_size, a size <= 0, levels < 0, a footprint that is not finite or not > 0, max_aniso outside 1 .. 16, a fov
 * that is not finite or outside (0, pi), a null or misaligned pointer, an output that overlaps an input or another output.
 * ZDR_E_UNSUPPORTED: more than 2^26 texels or 2^28 pixels; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_footprint_params) */
    int32_t tex_h, tex_w;
    int32_t width, height;             /* of the camera's image */
    zdr_camera camera;
} zdr_texel_footprint_params;
int zdr_texel_footprint(const zdr_texel_footprint_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                        float *out /* DEVICE tex_h x tex_w x 4 */, void *stream);
int zdr_texel_footprint_tangents(const zdr_texel_footprint_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                                 const float *tangents /* DEVICE tex_h x tex_w x 8 */, float *out /* DEVICE tex_h x tex_w x 4 */, void *stream);
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_gather_aniso_params) */
    int32_t tex_h, tex_w;
    int32_t width, height, levels;     /* of the image; levels as zdr_image_pyramid_params.levels */
    float footprint;
    int32_t max_aniso;                 /* 1 .. 16; 8 is the Python default */
} zdr_texel_gather_aniso_params;
int zdr_texel_gather_aniso(const zdr_texel_gather_aniso_params *params, const float *view, const float *footprint, const float *image,
                           const float *pyramid, float *color, void *stream);
int zdr_texel_gather_aniso_backward(const zdr_texel_gather_aniso_params *params, const float *view, const float *footprint,
                                    const float *d_color, float *d_image, float *d_pyramid, void *stream);

/* Gather plan: the adjoint of the three gathers above without a float atomic.  With the view held fixed a gather is a sparse linear map
 * from the image (and its pyramid) to the texture, and a view is fixed for as long as camera and geometry are.  A PLAN lays the
 * transpose of that map out once, as rows per destination pixel, and is then applied as a gather: a defined summation order, the same
 * bits from run to run, no hotspot where many texels tap one pixel.  The atomic adjoints above are unchanged.  No scene handle.
 *
 * Destinations (rows).  P0 = width height.  Pixel (x, y) of level 0 is row y width + x; pixel (x, y) of level l >= 1 is row
 * P0 + offset_l + y w_l + x, offset_l the level's place in the packed pyramid in pixels.  P = zdr_gather_plan_rows(params): P0 for the
 * bilinear filter, P0 + zdr_image_pyramid_bytes / 16 for mip and aniso (so an image without a level >= 1 has one row that stays empty).
 * Entries.  An entry is (texel: uint32, weight: float32), 8 bytes.  Every texel, in texel index order, enumerates exactly the taps its
 * scatter kernel touches, in this order, with the weight that kernel multiplies d_color by, operation for operation:
 *   filter 0, bilinear (zdr_texel_gather_backward)        taps 00, 01, 10, 11;  (w visible)
 *   filter 1, mip (zdr_texel_gather_mip_backward)         the four lower taps, ((w (1 - f)) visible); then, only where f != 0, the four
 *                                                         upper taps, ((w f) visible)
 *   filter 2, aniso (zdr_texel_gather_aniso_backward)     probe i = 0 .. N - 1 ascending, within a probe the lower taps, (((w (1 - f)) (1 / N))
 *                                                         visible), then where f != 0 the upper ones, (((w f) (1 / N)) visible)
 * w = (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty.  A texel whose visible is 0 or NaN has no entry; entries of weight 0 are kept;
 * taps that clamp onto the same pixel stay separate entries.  The ENTRY ID is the position in this enumeration; nnz is their number.
 * weight d_color[texel][c] is, bit for bit, the addend of the atomic adjoint.
 * Layout, CSR by row: row_start, P + 1 uint32 (row r holds the entries row_start[r] .. row_start[r + 1] - 1; row_start[P] = nnz);
 * entries, nnz x 8 bytes; within a row the entries are in ascending entry id.
 * Apply, zdr_gather_plan_apply, per channel c of a row with the entries e_0 .. e_{R-1}, in float32, nothing contracted:
 *   sixteen sub-sums: s_j = 0, then for k = j, j + 16, j + 32 .. in ascending order s_j = s_j + weight_k d_color[texel_k][c]
 *   the tree: s_j = s_j + s_{j+8} (j < 8); s_j = s_j + s_{j+4} (j < 4); s_j = s_j + s_{j+2} (j < 2); s_0 = s_0 + s_1
 *   a row of level 0 with R > 0: d_image[row] = d_image[row] + s_0 — ADDED INTO, as the atomic adjoints add; with R = 0 it is NOT
 *   TOUCHED, whatever bits it holds;  a row of the pyramid: d_pyramid[row - P0] = s_0 — WRITTEN, 0 for an empty row: the caller need
 *   not zero d_pyramid, and nothing in it is read.
 * The payload of a NaN is unspecified.  The full image gradient of mip and aniso is this call followed by zdr_image_pyramid_backward on
 * d_pyramid, as for the atomic adjoints.  d_pyramid may be null for the bilinear filter.
 *
 * Building a plan, once per (view, image size, filter and its parameters):
 *   1. zdr_gather_plan_count with a workspace of zdr_gather_plan_workspace_bytes(params, 0) bytes leaves nnz, a uint64, at the start of
 *      the workspace;
 *   2. the caller reads it — the ONE SYNCHRONISATION of a build, and the caller's: none of these calls synchronises or allocates;
 *   3. zdr_gather_plan_build with that nnz, a workspace of zdr_gather_plan_workspace_bytes(params, nnz) bytes (about 16 nnz plus what
 *      the sort asks for; the count's workspace may be this one or another), row_start (4 (P + 1) bytes) and entries (8 nnz bytes;
 *      non-null also when nnz is 0).  It counts again, writes the entries in entry-id order, sorts them STABLY by row and derives
 *      row_start.  nnz is meant to be the count's.  One below it drops the entries beyond it — the plan is then not the transpose; one
 *      above it still gives the right plan: the places no entry fills sort behind every row, row_start[P] is the true count and no
 *      row reaches the tail of `entries`, whose contents are unspecified.
 * The workspace's size needs a device to be present (the sort is asked for its own).  The same bits from build to build.
 * zdr_gather_plan_apply only enqueues (two launches) and can be captured in a HIP graph without a call before.  footprint, levels and
 * max_aniso are read as the filter's own call reads them (bilinear: none of them; mip: not max_aniso); `footprint_data` — the
 * footprint buffer — is read, and must be non-null, for aniso only.
 * All pointers are DEVICE pointers, 16-byte aligned.
 * ZDR_E_INVALID: a wrong struct_size, a size <= 0, levels < 0, a filter outside 0 .. 2, a footprint that is not finite or not > 0 (mip,
 * aniso), max_aniso outside 1 .. 16 (aniso), a null or misaligned pointer, an output or workspace that overlaps an input or another
 * output.  ZDR_E_UNSUPPORTED: more than 2^26 texels or 2^28 pixels, nnz above 2^31 - 1; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_gather_plan_params) */
    int32_t tex_h, tex_w;
    int32_t width, height;             /* of the image */
    int32_t filter;                    /* 0 bilinear, 1 mip, 2 aniso */
    int32_t levels;                    /* as zdr_image_pyramid_params.levels */
    float footprint;
    int32_t max_aniso;
} zdr_gather_plan_params;
size_t zdr_gather_plan_rows(const zdr_gather_plan_params *params);                          /* P; 0 = invalid */
size_t zdr_gather_plan_workspace_bytes(const zdr_gather_plan_params *params, uint64_t nnz);  /* 0 = invalid, or no device */
int zdr_gather_plan_count(const zdr_gather_plan_params *params, const float *view, const float *footprint_data, void *workspace, void *stream);
int zdr_gather_plan_build(const zdr_gather_plan_params *params, const float *view, const float *footprint_data, uint64_t nnz, void *workspace,
                          uint32_t *row_start, void *entries, void *stream);
int zdr_gather_plan_apply(const zdr_gather_plan_params *params, const uint32_t *row_start, const void *entries, const float *d_color,
                          float *d_image, float *d_pyramid, void *stream);

/* Camera gradients: the derivative of a gather in the view buffer, and the adjoint of the view buffer in the camera.  VISIBLE IS HELD
 * FIXED: neither the occlusion test nor the image-border test is differentiated (the interior derivative; biased where a silhouette
 * sweeps over texels).  Everything else in the view buffer is smooth in the camera, and the gathers are piecewise smooth in X, Y and
 * scale.  No scene handle, no ray, no float atomic; the calls above are unchanged.
 *
 * 1. zdr_texel_gather_dview: d_view (tex_h x tex_w x 8, every row OVERWRITTEN) from d_color (tex_h x tex_w x 4), for filter 0 (bilinear,
 * zdr_texel_gather) or 1 (mip, zdr_texel_gather_mip; pyramid, footprint and levels as that call takes them, not read for filter 0, where
 * pyramid may be null).  Filter 2 (aniso) is ZDR_E_UNSUPPORTED: its axis, N and B' would need derivatives of the footprint buffer.
 * Floats 2 (d_X), 3 (d_Y) and, mip, 6 (d_scale) carry values, the rest are 0.  Where visible is 0 or NaN the row is eight zeros and
 * neither the image, the pyramid nor d_color of that texel is read.  Otherwise, for a sample of level l with the taps c00, c01, c10, c11
 * and the fractions tx, ty exactly as the forward forms them (X 2^-l, Y 2^-l; level 0 for the bilinear filter), per channel
 *   a = c01 - c00,  b = c11 - c10,  gx = (a + (b - a) ty) 2^-l,  gy = (bot - top) 2^-l,   top, bot the forward's two lerps,
 * the scaling exact.  Mip: g = lo + (hi - lo) f for gx and gy as the forward blends the colours; where f == 0 the upper level is not read.
 *   d_X = visible (((d_color_0 gx_0 + d_color_1 gx_1) + d_color_2 gx_2) + d_color_3 gx_3),   d_Y likewise with gy,
 * in float32, uncontracted.  Taps that clamp onto one pixel give a = 0 by themselves: this is the derivative of the forward as it is
 * implemented, and at an integer fx the right-hand one, as the floor dictates.  Where the level split moves with scale — 0 < f < 1, which
 * implies s = scale footprint > 1 and l0 < L; f == 1 is log2f's clamp —
 *   d_scale = visible (dot(d_color, hi - lo) (footprint / (s ln 2))),   dot as above, hi and lo the two levels' colours, ln 2 as a float,
 * so that the result is the derivative of the forward and not of a surrogate with frozen levels.  Where s <= 1 the mip result is the
 * bilinear one bit for bit.  One thread per texel, no workspace: the same bits from run to run.
 *
 * 2. zdr_texel_view_backward: d_camera, 10 floats in zdr_camera's order (fov, origin, target, up), OVERWRITTEN, from d_view (tex_h x
 * tex_w x 8) and the texel buffer the view was made from (normal n, texel_size, position p and reach are read, as in the forward), with
 * the params of zdr_scene_texel_view.  For every SHADED texel (the forward's rule), with the frame and the quantities of that call,
 * v = p - o, z, dist, wi, cosine, a = v.right, b = v.upp, and g_1 .. g_6 = floats 1 .. 6 of its d_view row (floats 0 and 7 are ignored;
 * the row of a texel that is not shaded is not read):
 *   kx = half_w / (z tan),  ky = half_h / (z (tan aspect)),  qx = a / z,  qy = b / z           dX/da = kx, dY/db = -ky
 *   ga = g_2 kx,  gb = -(g_3 ky),  gxy = g_3 (ky qy) - g_2 (kx qx)                             dX/dz = -kx qx, dY/dz = ky qy
 *   gz = (g_4 + gxy) - (g_6 scale) / z,   gt = (gxy z - g_6 scale) / tan                       dscale/dz = -scale / z, d./dtan = (z / tan) d./dz
 * where z > 0, and ga = gb = gt = 0, gz = g_4 elsewhere (there X, Y and scale are the constant 0);
 *   gv = ((gz fwd + ga right) + gb upp) - ((g_1 / dist) (n - cosine wi) + g_5 wi)               dcosine/dv = -(n - cosine wi) / dist, ddist/dv = -wi
 * and the texel's 13 partial derivatives are  d_o = -gv,  d_fwd = gz v,  d_right = ga v,  d_upp = gb v,  d_tan = gt,  float32, uncontracted.
 * Their sums over the texels are taken in FLOAT64 (the terms cancel, and the chain rule below differences the totals once more), in a
 * fixed order: G = 256 R lanes, R = min(ceil(ntexels / 256), 1024); lane g adds the texels g, g + G, g + 2G .. in ascending order; within
 * each wave of 64 consecutive lanes, lane i adds lane i + 32 to itself, then i + 16, 8, 4, 2, 1; the four waves of a workgroup of 256
 * consecutive lanes are added in wave order, which gives one partial row per workgroup in the workspace; sixteen sub-sums add the rows
 * r, r + 16, r + 32 .. ascending, and are added in order.  One lane takes the totals through the frame — d = target - origin, fwd = d / |d|,
 * c = fwd x up, right = c / |c|, upp = right x fwd, tan = tan(fov / 2) — in float64, the frame formed once more in float64 from the
 * camera's floats (the Jacobian of the exact map: what the projections remove, such as d_up along up, is then 0 to float64's rounding):
 *   g_right += fwd x g_upp,  g_fwd += g_upp x right,  g_c = (g_right - right (right . g_right)) / |c|,  g_fwd += up x g_c,
 *   d_up = g_c x fwd,  d_target = (g_fwd - fwd (fwd . g_fwd)) / |d|,  d_origin = g_o - d_target,  d_fov = g_tan (1 + tan^2) / 2,
 * rounded to float32 once.  A degenerate frame (up parallel to fwd) gives NaN, as the forward does.  `workspace`: at least
 * zdr_texel_view_backward_workspace_bytes(tex_h, tex_w) bytes (0 = invalid size; 128 R), contents irrelevant: nothing is read that
 * the call did not write.  No float atomic, no dependence on the launch order: the same bits from run to run.
 *
 * All pointers are DEVICE pointers, 16-byte aligned.  The calls only enqueue on `stream` (one launch, two launches): they never allocate
 * and never synchronise, and can be captured in a HIP graph without a call before.
 * ZDR_E_INVALID: a null or misaligned pointer, a wrong struct_size, a size <= 0, levels < 0, a filter outside 0 .. 2, a footprint that is
 * not finite or not > 0 (mip), a fov that is not finite or not in (0, pi), an output or workspace that overlaps an input or the other.
 * ZDR_E_UNSUPPORTED: filter 2; more than 2^26 texels or 2^28 pixels; a library linked without these kernels. */
typedef struct {
    uint32_t struct_size;              /* = sizeof(zdr_texel_gather_dview_params) */
    int32_t tex_h, tex_w;
    int32_t width, height;             /* of the image */
    int32_t filter;                    /* 0 bilinear, 1 mip */
    int32_t levels;                    /* as zdr_image_pyramid_params.levels */
    float footprint;
} zdr_texel_gather_dview_params;
int zdr_texel_gather_dview(const zdr_texel_gather_dview_params *params, const float *view, const float *image, const float *pyramid,
                           const float *d_color, float *d_view, void *stream);
size_t zdr_texel_view_backward_workspace_bytes(int32_t tex_h, int32_t tex_w);   /* 0 = invalid size */
int zdr_texel_view_backward(const zdr_texel_view_params *params, const float *texel_aovs /* DEVICE tex_h x tex_w x 16 */,
                            const float *d_view /* DEVICE tex_h x tex_w x 8 */, float *d_camera /* DEVICE 10 floats */, void *workspace,
                            void *stream);

/* Path statistics of one forward pass over the shard: counters[8] (HOST, written
 * after an internal synchronise) = camera samples, closest-hit rays, closest rays that hit,
 * shadow rays (one per shaded vertex, prb.py:59), shaded vertices, emitter hits via BSDF sampling, NaN-dropped samples,
 * shadow rays actually traced (the BVH kernels skip those whose light sample carries nothing). */
int zdr_render_stats(zdr_scene *scene, const zdr_render_params *params, const float *material,
                     uint64_t counters[8], void *stream);

/* The kernels carry watchdogs that can end work early instead of spinning on the GPU (a persistent wave that makes
 * no progress; a BVH walk past its iteration budget).  They never trip on valid inputs; if one does it sets a sticky
 * bit in a device error word, and the images / gradients produced since the last check are INCOMPLETE.
 * zdr_scene_check synchronises `stream`, returns ZDR_E_HIP (message in zdr_last_error) if the word is set, and
 * clears it.  zdr_render_stats checks by itself; with the environment variable ZDR_CHECK=1 every render call does
 * (one synchronise per call).  The reference has no counterpart: LuisaCompute raises from luisa.synchronize()
 * (render.py:172,198). */
int zdr_scene_check(zdr_scene *scene, void *stream);

/* LuisaCompute Accel.trace_closest / trace_any (prb.py:25,59) as batch queries, for testing the
 * acceleration structure.  DEVICE rays: n x 8 {o[3], tmin, d[3], tmax}.
 * inst_prim: n x 2 int32 (-1,-1 on miss); bary_t: n x 3 float32 {u, v, t}; occluded: n int32. */
int zdr_trace_closest(zdr_scene *scene, const float *rays, uint32_t n, int32_t *inst_prim, float *bary_t, void *stream);
int zdr_trace_any(zdr_scene *scene, const float *rays, uint32_t n, int32_t *occluded, void *stream);

/* Sampler values as the kernels draw them, for bit-exact comparison with the oracle
 * (BASELINE.json: "sample indices bit-exact").  For each of n queries {px, py, sample_index}
 * (DEVICE int32 n x 3) writes 2 + 8*nvert float32 to out (DEVICE, stride 2 + 8*nvert): next2f,
 * then per vertex next,next,next2f,next,next2f and — for vertices k >= rr_depth — next
 * (SURVEY App. A.8); unused slots are 0. */
int zdr_sampler_dump(zdr_scene *scene, int32_t sampler, uint32_t seed, uint32_t spp, const int32_t *queries,
                     uint32_t n, int32_t nvert, int32_t rr_depth, float *out, void *stream);

/* The same draws, produced THE WAY THE PATH KERNELS PRODUCE THEM: on every BASELINE configuration (CMJ, power-of-two spp
 * <= 65536 and strata grid) the path kernels do not call next() / next2f() one by one (corrmj.py:95-117) but draw a
 * vertex's seven numbers at once with two Kensler permutations per register (csrc/sampler.h, cmj_vertex_samples) and the
 * Russian-roulette number from an index permuted alongside (cmj_next_with_index).  This entry point runs exactly that code
 * — and the one-by-one calls where the kernels fall back to them — so that "sample indices bit-exact" is asserted on the
 * instructions the renders execute.  `integrator` = ZDR_PATH or ZDR_DIRECT: the direct kernels pack the PIXEL's 2-D draw
 * (an index pass + one packed pass for its two strata, csrc/sampler.h cmj_next2_packed) and draw the vertex's numbers one
 * by one; the path kernels draw the pixel's numbers one by one and pack the vertex's (each kernel keeps the form that
 * its register budget pays for: csrc/integrators.h, pixel_ray).  Other arguments and the output
 * layout as zdr_sampler_dump; *batched (HOST, may be NULL) receives 0 for the fallback and non-zero when the packed route was
 * taken: 2 when the path kernels also permute the four strata of a vertex's two 2-D draws in one pass, one per byte (strata
 * grid of at most 16 x 16, i.e. spp <= 256: csrc/sampler.h, permutation_element4), else 1. */
int zdr_vertex_sampler_dump(zdr_scene *scene, int32_t integrator, int32_t sampler, uint32_t seed, uint32_t spp,
                            const int32_t *queries, uint32_t n, int32_t nvert, int32_t rr_depth, float *out,
                            int32_t *batched, void *stream);

/* Per-path traces of the path integrator, for comparing the kernels with the oracle PATH BY PATH (glossy materials
 * amplify last-ulp differences, so whole-image statistics alone cannot tell a flipped branch from wrong arithmetic).
 * For each of n queries {px, py, sample_index} (DEVICE int32 n x 3) the camera sample is walked with the device
 * functions of the path kernels (prb.py:19-88) and swept like the backward kernel (prb.py:92-187); `params` as for
 * zdr_render_backward (its seed is used as it is), d_image the cotangent (DEVICE, or NULL = ones).
 * out (DEVICE float32, n x (8 + 24 maxv), 1 <= maxv <= 16):
 *   header  {bits(nvert), L.rgb — the sample's radiance before the clamp of integrator.py:26 —, 0, Li.rgb of the emitter that ended it}
 *   vertex  {bits(inst), bits(prim), uv.xy, bits(flags), pdf_bsdf, wi.xyz (world), beta.rgb leaving the vertex,
 *            grad.rgba (what the backward pass scatters at uv for this vertex), NEE radiance.rgb, 0 x 5}
 *   flags = light sample accepted | path went on << 1 | Russian roulette kind << 2 (0 none, 1 stochastic, 2 renormalising).
 * A query whose pixel lies outside the image or whose sample_index >= spp yields an all-zero row. */
int zdr_path_dump(zdr_scene *scene, const zdr_render_params *params, const float *material, const float *d_image,
                  const int32_t *queries, uint32_t n, int32_t maxv, float *out, void *stream);

/* The FUSED walk of the BVH path kernels as a batch query (test hook): what a path vertex hands the acceleration structure — a shadow
 * ray and a continuation ray per lane, walked in one loop in which lanes that are through take subtrees from lanes that are not
 * (csrc/accel.h, BvhAccel::shadow_and_closest / walk_steal) — where zdr_trace_closest / zdr_trace_any walk one ray per lane without
 * stealing.  Ray pair i is lane i % 64 of wave i / 64: the caller chooses who shares a wave, hence who can steal from whom; the lanes
 * of the last wave beyond n take part without a ray.  shadow_rays / next_rays: DEVICE n x 8 {o[3], tmin, d[3], tmax}; tmin / tmax of
 * next_rays are ignored (0 and 1e30, as the path kernels pass them).  need (DEVICE, n): bit 0 the pair has a shadow ray, bit 1 a
 * continuation ray.  backward_layout != 0: the LDS layout of the backward path kernel (fewer stack entries in LDS) instead of the
 * forward one's.  occluded (n): 1 when the shadow ray is blocked, 0 without bit 0; inst_prim / bary_t as zdr_trace_closest, (-1, -1)
 * and (0, 0, 1e30) on a miss or without bit 1.  The answers are those of zdr_trace_any / zdr_trace_closest for the same rays.
 * The call compiles the fused walk into a kernel of its own: it checks the routine's logic, not the copy of it inlined into the
 * path kernels (that is what the path-by-path parity tests run).  BVH scenes only: ZDR_E_UNSUPPORTED on a brute-force scene.
 * n = 0 does nothing. */
int zdr_trace_fused(zdr_scene *scene, const float *shadow_rays, const float *next_rays, const int32_t *need, uint32_t n,
                    int32_t backward_layout, int32_t *occluded, int32_t *inst_prim, float *bary_t, void *stream);

/* The shading math point by point (test hook): row i (lane i of a kernel of its own) calls the very device functions the path kernels
 * call at a vertex — csrc/microfacet.h (ggx_terms, ggx_brdf_from, ggx_pdf_from, ggx_dfdr_from, ggx_sample / sample_wm_disk), brdf_grad
 * and the shading frame (make_onb, to_local, to_world) — on inputs the caller chooses; no geometry is read, `scene` only names the
 * device.  in / out: DEVICE float32, n rows of 16 floats each; the floats of a row that are not listed are ignored (in) or written
 * as 0 (out); rows n and beyond are not touched.  Directions are LOCAL (z = shading normal) and taken as they are, not normalised.
 *   ZDR_SHADING_EVAL    in  {wo[3], wi[3], roughness, diffuse[3], ct[3]}
 *                       out {f[3] (BRDF times cosine), pdf, dfdr = d f / d roughness, dlnpdf_dr, t, D (of GgxTerms: t = nh^2 (a2 - 1) + 1,
 *                            D = a2 / (pi t^2)), brdf_grad(wi.z / pi, dfdr, ct)[4]}
 *   ZDR_SHADING_SAMPLE  in  {wo[3], roughness, diffuse[3], u_lobe, u_dir[2]}
 *                       out {wi_local[3], pdf, (f * rcp(pdf))[3] — the throughput factor as sample_bsdf forms it —, dfdr, dlnpdf_dr,
 *                            1.0 if wi_local.z < 1e-4 (the path stops, prb.py:74) else 0.0, t, D}; everything after wi_local is evaluated at it
 *   ZDR_SHADING_FRAME   in  {n[3] (unit normal), d[3]}
 *                       out {tangent[3], binormal[3], normal[3] of make_onb(n), to_local(onb, d)[3], to_world(onb, to_local(onb, d))[3]}
 * The call only enqueues on `stream`.  ZDR_E_INVALID for a null scene, an unknown mode, or null in / out with n > 0; n = 0 does nothing.
 * It checks the functions' arithmetic as compiled into this kernel, not the instances inlined into the path kernels (the path-by-path
 * parity tests run those). */
enum { ZDR_SHADING_EVAL = 0, ZDR_SHADING_SAMPLE = 1, ZDR_SHADING_FRAME = 2 };
int zdr_shading_dump(zdr_scene *scene, int32_t mode, const float *in, uint32_t n, float *out, void *stream);

/* The light side of a path vertex point by point (test hook): row i (lane i of a kernel of its own, k_light_dump) calls the device
 * functions the kernels sample and weigh lights with — csrc/scene.h: sample_light (sample_uniform_triangle, light_pdf, sample_alias_table
 * behind it), sample_light_pdf, env_sampled_light_pdf, env_lookup, uv_to_direction, direction_to_uv, env_pdf_scale, balanced_heuristic,
 * offset_ray_origin, surface_interact; csrc/integrators.h: tent_warp1 — on inputs the caller chooses, with the scene's own light table,
 * environment map and acceleration structure.  in / out: DEVICE float32, n rows of 16 floats each; floats not listed are ignored (in)
 * or written as 0 (out); rows n and beyond are not touched.  Nothing is normalised on the way in.
 *   ZDR_LIGHT_SAMPLE    in  {origin[3], u_pick, u_prim, u_pt[2]}
 *                       out {wi[3], dist, pdf, eval[3], env_uv[2] (the map coordinates of an environment sample; -1, -1 when the mesh
 *                            branch or the no-light branch ran), bits(mesh_light) (list index of a mesh light sampled from its front, else -1)}
 *                       sample_light<ENV, true> with the row's numbers as its draws; ENV = the scene has a map.  A scene without any
 *                       light takes the n <= 0 branch.
 *   ZDR_LIGHT_PDF       in  {origin[3], p[3], bits(inst), bits(tri)}   tri: index of the triangle in the scene's input order
 *                       out {sample_light_pdf<ENV, true>, sample_light_pdf<ENV, false>, bits(slot)} at the slot the scene keeps the
 *                            triangle in; {NaN, NaN, -1} and nothing read when inst or tri names nothing of the scene
 *   ZDR_LIGHT_ENV       in  {d[3], u, v}   (scenes with a map only)
 *                       out {direction_to_uv(d)[2], env_sampled_light_pdf(d), env_lookup(direction_to_uv(d))[3], uv_to_direction(u, v)[3],
 *                            direction_to_uv(uv_to_direction(u, v))[2], env_pdf_scale(v, number of lights)}
 *   ZDR_LIGHT_MISC      in  {a, b, p[3], n[3], u[2], t}
 *                       out {balanced_heuristic(a, b), offset_ray_origin(p, n)[3], sample_uniform_triangle(u)[3], tent_warp1(t)}
 *   ZDR_LIGHT_INTERACT  in  {o[3], d[3], tmin, tmax}
 *                       out {bits(inst), bits(prim), u, v, t, p[3], uv[2], ns[3], ng[3]}: the closest hit of the scene's acceleration
 *                            structure, reported as zdr_trace_closest reports it (-1, -1, 0, 0, tmax and zeros on a miss), and
 *                            surface_interact<true> at it.  ZDR_LIGHT_INTERACT_WIDE: the same with surface_interact<false>.
 * The call only enqueues on `stream`.  ZDR_E_INVALID for a null scene, an unknown mode, ZDR_LIGHT_ENV on a scene without a map, or null
 * in / out with n > 0; n = 0 does nothing.  It checks the functions as compiled into this kernel, not the instances inlined into the
 * render kernels (the path-by-path and image parity tests run those). */
enum { ZDR_LIGHT_SAMPLE = 0, ZDR_LIGHT_PDF = 1, ZDR_LIGHT_ENV = 2, ZDR_LIGHT_MISC = 3, ZDR_LIGHT_INTERACT = 4, ZDR_LIGHT_INTERACT_WIDE = 5 };
int zdr_light_dump(zdr_scene *scene, int32_t mode, const float *in, uint32_t n, float *out, void *stream);

/* The bilinear texture lookup row by row (test hook): row i (lane i of a kernel of its own) calls the device functions the kernels shade
 * with — read_bsdf and read_bsdf_in, each with 32-bit byte offsets ("narrow") and with 64-bit addresses ("wide"), and env_lookup of the
 * scene's environment map — at a uv the caller chooses, outside [0, 1] included.  materials / dims / nmat: as zdr_render_*_materials takes
 * them (DEVICE packed float4 texels; HOST nmat x {h, w}; 1 <= nmat <= ZDR_MAX_MATERIALS).  The scene's material slots are not consulted.
 * rows (DEVICE float32, n x 4): {u, v, bits(material index), ignored}.
 * out  (DEVICE float32, n x 20): {read_bsdf narrow[4], read_bsdf wide[4], read_bsdf_in narrow[4], read_bsdf_in wide[4],
 *                                 env_lookup(u, v)[3] (zeros when the scene has no map), 0}.
 * ZDR_E_INVALID, before anything is launched or written, for a null scene or dims, nmat outside [1, 16], a size < 1, a material index
 * outside [0, nmat), or null materials / rows / out with n > 0; n = 0 does nothing.  The rows are read back and checked on the host, so the
 * call synchronises `stream` and cannot be captured into a graph (ZDR_E_UNSUPPORTED on a capturing stream).
 * It checks the functions as compiled into this kernel, not the instances inlined into the render kernels (the parity tests run those). */
int zdr_texture_lookup(zdr_scene *scene, const float *materials, const int32_t *dims, uint32_t nmat, const float *rows, uint32_t n,
                       float *out, void *stream);

/* The lookup's adjoint row by row (test hook): the staging-cell scatter of the backward kernels and the fold into the gradient texture,
 * on gradients, uvs and ballots the caller chooses.  The call does what a backward call does around its kernel: it lays the staging
 * cells out and zeroes them with the code the render calls use, launches a kernel of its own that runs scatter_queue_init[_cells], the
 * pushes and scatter_finish (csrc/scene.h), and then the fold of the backward calls (k_cells_to_grad / k_material_cells_to_grad), which
 * ADDS to what the gradient buffers hold.
 * rows (DEVICE float32, n x 8): {u, v, g[4], bits(material index), ignored}; a negative material index is an inactive row.
 * One wave per block; wave b makes `rounds` pushes, and in round r its lane l holds row 64 (b rounds + r) + l and calls scatter_push
 * with active = the row exists (< n) and is active: the caller decides every ballot and with it every flush of the queue.
 * form: the template instance of the render kernels that runs —
 *   ZDR_SCATTER_SINGLE     one material (nmat = 1), as zdr_render_backward: copies from the size of its cell grid;
 *   ZDR_SCATTER_TABLE      a material table, as zdr_render_backward_materials: the per-material cell layout;
 *   ZDR_SCATTER_TABLE_ENV  a material table (nmat <= 15) and the scene's environment map as entry 15, as zdr_render_backward_materials_env:
 *                          a row whose material index is 15 is a gradient of the map at (u, v), in env_lookup's footprint, and lands in d_env.
 * dims / nmat: as above.  d_materials: DEVICE, the packed gradient, every material's texels x 4.  d_env: DEVICE (env_h, env_w, 4), the third
 * form only (ignored otherwise).  copies (HOST, ZDR_MAX_MATERIALS int32, or NULL): receives how many copies of its staging cells each
 * material was given (entry 15: the map's, third form; unused entries 0) — which of the storage regimes of csrc/scene.h the call ran in.
 * ZDR_E_INVALID, before anything is launched or written, for a null scene or dims, an unknown form, nmat outside [1, 16] (or != 1, or > 15,
 * as the form demands), a size < 1, rounds outside [1, 65536], the third form on a scene without a map, a material index >= nmat (other
 * than 15 in the third form), or null rows / d_materials / d_env (third form) with n > 0.  n = 0 reports the copies and does nothing else.
 * The rows are read back and checked on the host, so the call synchronises `stream` and cannot be captured (ZDR_E_UNSUPPORTED).
 * It checks the functions as compiled into this kernel, not the instances inlined into k_path_bwd, k_simple and k_aov_bwd (the rendered
 * gradient parity tests run those); the fold kernels are the very kernels the backward calls launch. */
enum { ZDR_SCATTER_SINGLE = 0, ZDR_SCATTER_TABLE = 1, ZDR_SCATTER_TABLE_ENV = 2 };
int zdr_texture_scatter(zdr_scene *scene, int32_t form, const int32_t *dims, uint32_t nmat, const float *rows, uint32_t n, uint32_t rounds,
                        float *d_materials, float *d_env, int32_t *copies, void *stream);

/* Host-only: builds the acceleration structure exactly as zdr_scene_create does and returns it,
 * without touching a GPU, so that the CPU test-suite can run an emulation of the device traversal
 * on the very data the kernels read (tests/test_bvh_emulation.py).  tri_xyz: ntris x 9 world-space
 * corners.  nodes_out: nodes_cap x 16 floats (BVH4 node = 64 bytes, layout in csrc/scene.h);
 * order_out[slot] = input triangle; isect_out: ntris x 12 floats (plane-form records, slot order).
 * Brute force (ZDR_ACCEL_BRUTE, or AUTO with <= 64 triangles): there are no nodes; *nnodes receives the number Q of
 * planar convex quads the walk merged out of coplanar triangle pairs — slots 2q and 2q + 1 for q < Q, the other
 * triangles after them — and the records of a quad's two triangles start at the corner OPPOSITE the shared edge;
 * *stack_entries receives how many of the quads are parallelograms (they come first; the walk tests them in pairs with
 * the first triangle's u, v and 1 - u, 1 - v) (tests/test_brute_quads.py).  (zdr_scene_create additionally orders the
 * primitives WITHIN each of these groups so that those a shadow segment can meet come first — zdr_debug_never_occluders —
 * which needs the lights and is not reproduced here.)  A corner that is not finite or beyond ZDR_MAX_COORD is refused as
 * zdr_scene_create refuses it: ZDR_E_INVALID, the message names the triangle and which of its three corners. */
int zdr_debug_build_accel(const float *tri_xyz, uint32_t ntris, int accel, float *nodes_out, uint32_t nodes_cap,
                          uint32_t *nnodes, uint32_t *stack_entries, int32_t *order_out, float *isect_out);

/* Host-only: which triangles can never lie between a surface point of the scene and a point of a light, i.e. can be left out of
 * the shadow-segment walk of next-event estimation (prb.py:57-59; csrc/zdr_api.cpp, never_occluders: the triangle's plane supports
 * the whole scene and the lights keep a distance from it that makes a hit inside (tmin, tmax) impossible).  The brute-force accel
 * skips the pairs of the pair walk whose primitives all qualify.  tri_xyz: ntris x 9 world-space corners; is_light_tri: ntris flags;
 * never_out: ntris flags (tests/test_brute_quads.py). */
int zdr_debug_never_occluders(const float *tri_xyz, uint32_t ntris, const uint8_t *is_light_tri, uint8_t *never_out);

#ifdef __cplusplus
}
#endif
#endif
