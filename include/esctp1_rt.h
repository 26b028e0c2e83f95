/*
 * esctp1_rt.h -- C ABI of the MI355X-native renderer that replaces the per-pixel render
 * loop of pg42819/EscTp1RayTracer.
 *
 * Plain C: pointers, sizes and PODs only (no C++ / torch types), so the reference's
 * C++ host (or any FFI: ctypes, cgo, JNI) can bind it.  Each entry point cites the
 * reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - every function returning int returns ESC_OK (0) or a negative ESC_ERR_* code;
 *     esc_last_error() gives the thread-local message.  No exception crosses this ABI
 *     (the reference throws std::runtime_error, main.cpp:490-534, sceneloader.cpp:27-30).
 *   - images are interleaved RGB, pixel (w,h) at index (h*W + w)*3, h = 0 is the BOTTOM
 *     row (main.cpp:784-788 `image[h*W+w]`, flat form main.cpp:667-673).
 *   - all host buffers are caller-owned; the library keeps no pointer after a call returns
 *     unless stated.
 *   - one esc_context per host thread / per GPU; calls on one context are not re-entrant.
 */
#ifndef ESCTP1_RT_H
#define ESCTP1_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  ESC_OK = 0,
  ESC_ERR_INVALID = -1, /* bad argument / shape mismatch */
  ESC_ERR_HIP = -2,     /* HIP runtime error (message carries hipGetErrorString) */
  ESC_ERR_IO = -3,      /* file could not be opened / written */
  ESC_ERR_PARSE = -4,   /* OBJ/MTL rejected (mirrors sceneloader.cpp:27-30,67-70 throws) */
  ESC_ERR_NOMEM = -5,
  ESC_ERR_NO_DEVICE = -6, /* no usable gfx950 device: the product has NO CPU fallback */
  ESC_ERR_RCCL = -7       /* RCCL missing or an ncclResult_t != ncclSuccess (message carries
                             ncclGetErrorString) */
};

const char *esc_last_error(void);
/* "esctp1raytracer_amd <ver> gfx950 hip" */
const char *esc_version(void);

/* ------------------------------------------------------------------------------------
 * Host scene  == tracer::scene (src/scene/scene.h:8-44)
 * ---------------------------------------------------------------------------------- */
typedef struct esc_scene esc_scene;

/* tracer::scene::Material, scene.h:11-18, as 13 floats: ka[3] kd[3] ks[3] ke[3] Ns */
#define ESC_MATERIAL_FLOATS 13

esc_scene *esc_scene_new(void);
void esc_scene_free(esc_scene *scene);

/* Append one tracer::scene::Geometry (scene.h:20-31): de-indexed vertices, optional
 * per-vertex normals (n_normals == 0 => none), face_index triples into `vertex`.
 * The geometry is a light source iff dot(ke,ke) > 0 (sceneloader.cpp:63-64,102-104).
 * Coordinates must be finite and face indices in range (ESC_ERR_INVALID otherwise).
 * Returns the new geomID (>= 0) or a negative error. */
int esc_scene_add_geometry(esc_scene *scene, const float *vertex, int32_t n_vertices,
                           const float *normals, int32_t n_normals, const uint32_t *face_index,
                           int32_t n_faces, const float material[ESC_MATERIAL_FLOATS]);

/* EXTENSION (not in the reference): analytic spheres, cx cy cz r each,
 * one material per sphere.  Tie order: after every triangle, then by sphere index. */
int esc_scene_add_spheres(esc_scene *scene, const float *spheres_xyzr, const float *materials,
                          int32_t n_spheres);

/* model::loadobj (src/scene/sceneloader.h:10, sceneloader.cpp:14-106): OBJ + MTL ->
 * one geometry per OBJ shape, vertices de-indexed 3 per face, material = first face's
 * material, normals normalised on load.  Appends to `scene`. */
int esc_scene_load_obj(esc_scene *scene, const char *obj_path);

/* Synthetic scenes of BASELINE.json's configs (generator splitmix64):
 *   "c2" 100 spheres, "c3" 1k spheres, "c4" 10k spheres, "c5" 100,352-triangle heightfield,
 *   each with the 2-triangle floor and one single-triangle light.  n_override > 0 replaces
 *   the primitive count (spheres, or heightfield quads per side for c5). */
int esc_scene_synthetic(esc_scene *scene, const char *config, int32_t n_override);
/* eye / look-at of the synthetic configs: (0,3,6) -> (0,2,-8) */
void esc_synthetic_view(float eye[3], float look[3]);

/* introspection (tests, bindings) */
typedef struct {
  int32_t n_geometry;
  int32_t n_lights;
  int32_t n_triangles; /* sum of faces */
  int32_t n_spheres;
} esc_scene_info;
int esc_scene_get_info(const esc_scene *scene, esc_scene_info *info);
/* counts[3] = n_vertices, n_normals, n_faces */
int esc_scene_geometry_counts(const esc_scene *scene, int32_t geom, int32_t counts[3]);
int esc_scene_geometry_copy(const esc_scene *scene, int32_t geom, float *vertex, float *normals,
                            uint32_t *face_index, float material[ESC_MATERIAL_FLOATS]);
int esc_scene_light_sources(const esc_scene *scene, int32_t *geom_ids /* [n_lights] */);
int esc_scene_spheres_copy(const esc_scene *scene, float *spheres_xyzr, float *materials);

/* EXTENSION: transmission of a material, for esc_trace_rays_ex / esc_render_traced_ex.  A side table
 * next to the 13-float material (whose layout does not change): tf[3], the transmission filter
 * (MTL `Tf`), and ni, the index of refraction (MTL `Ni`).  The default is tf = 0, ni = 1: opaque.
 * Any float value is accepted, NaN included; the bounce rule at esc_trace_options says what it does.
 * esc_scene_load_obj sets tf = Tf, ni = Ni on a geometry iff its material's `illum` is 4, 6, 7 or 9
 * (the MTL illumination models with transparency or refraction); under any other model the geometry
 * stays opaque whatever its Tf.  An index out of range is ESC_ERR_INVALID. */
#define ESC_TRANSMISSION_FLOATS 4 /* tf[3], ni */
int esc_scene_set_geometry_transmission(esc_scene *scene, int32_t geom, const float tr[ESC_TRANSMISSION_FLOATS]);
int esc_scene_get_geometry_transmission(const esc_scene *scene, int32_t geom, float tr[ESC_TRANSMISSION_FLOATS]);
/* spheres first .. first + n - 1; tr: n x 4 */
int esc_scene_set_sphere_transmission(esc_scene *scene, int32_t first, int32_t n, const float *tr);
/* tr: n_spheres x 4 */
int esc_scene_get_sphere_transmission(const esc_scene *scene, float *tr);

/* ------------------------------------------------------------------------------------
 * Camera == tracer::camera (src/scene/camera.h:7-41); ctor arithmetic runs on the host
 * ---------------------------------------------------------------------------------- */
typedef struct {
  float origin[3];
  float lower_left_corner[3];
  float horizontal[3];
  float vertical[3];
} esc_camera;

/* camera.h:16-29.  aspect = float(W)/H at the call site (main.cpp:548). */
void esc_camera_init(esc_camera *cam, const float lookfrom[3], const float lookat[3],
                     const float vup[3], float vfov, float aspect);

/* ------------------------------------------------------------------------------------
 * ISPC-compatible flat scene == FlatScene (src/simplify/flatten_iscp.h:9-13) with the
 * structs of src/ispc/ispc_helpers.h:16-48.  Layouts are byte-identical to what the
 * ispc compiler emits into trace_ispc.h for those declarations.
 * ---------------------------------------------------------------------------------- */
typedef struct ispc_triangle {
  float vertices[3][3];
  float normals[3][3];
  int32_t prim_id;
  int32_t geom_id;
  int32_t has_normals;
  int32_t is_light;
  float ka[3];
  float kd[3];
  float ks[3];
  float ke[3];
  float Ns;
} ispc_triangle; /* 140 bytes */

typedef struct ispc_light {
  int32_t geom_id;
  int32_t *light_faces; /* indexes into light_triangles[] */
  int32_t num_light_faces;
} ispc_light; /* 24 bytes on LP64 */

typedef struct ispc_cam {
  float lookfrom[3];
  float lookat[3];
  float vup[3];
  float vfov;
  float aspect;
} ispc_cam; /* 44 bytes */

typedef struct esc_flat_scene esc_flat_scene;
/* flatten_scene_ispc (flatten_iscp.cpp:35-111).  sort_by_centroid_x != 0 reproduces the
 * reference's std::sort at flatten_iscp.cpp:110 (it permutes primitive indices: equal-t ties and,
 * with >= 2 lights, the first occluder in index order -- quirk S3 -- can change);
 * 0 keeps (geometry, face) order == the scalar path's order and image.  Unlike the reference
 * (dangling vector, defect I4) the light_faces arrays stay valid until esc_flat_free. */
int esc_flatten_ispc(const esc_scene *scene, int32_t sort_by_centroid_x, esc_flat_scene **out);
void esc_flat_free(esc_flat_scene *flat);
ispc_triangle *esc_flat_triangles(esc_flat_scene *flat, int32_t *n);
ispc_triangle *esc_flat_light_triangles(esc_flat_scene *flat, int32_t *n);
ispc_light *esc_flat_lights(esc_flat_scene *flat, int32_t *n);
/* new_ispc_cam (flatten_iscp.cpp:117-128) */
void esc_new_ispc_cam(ispc_cam *cam, const float lookfrom[3], const float lookat[3],
                      const float vup[3], float vfov, float aspect);

/* ------------------------------------------------------------------------------------
 * THE DROP-IN: same symbol, argument list and image convention as the ISPC export
 *   src/ispc/trace.ispc:86-92, called at src/main.cpp:619-624
 * (the generated header declares it `extern "C"` inside namespace ispc with `ispc_cam &`;
 * a C++ reference is a pointer in the C ABI).  Semantics = the reference's SCALAR path
 * (main.cpp:698-791) on the flat arrays in the order given; the image is OVERWRITTEN (the
 * reference accumulates into uninitialised memory, defect I3).  Synchronous; renders on
 * device 0 (or $ESC_DEVICE); errors are reported on stderr and leave the image zeroed,
 * because the replaced function returns void.  Multi-face lights use the counter-based
 * face choice below with seed 0.  $ESC_TRACE_STAGE=bvh renders through the opt-in
 * acceleration structure (ESC_STAGE_BVH below) -- same image.
 * The reference's C++ host gets the `ispc::trace(..., ispc_cam &, ...)` form of this
 * declaration from include/trace_ispc.h (the replacement for the ISPC-generated header).
 * ---------------------------------------------------------------------------------- */
#ifndef ESC_NO_TRACE_DECL /* include/trace_ispc.h declares it with `ispc_cam &` in namespace ispc */
void trace(int32_t image_width, int32_t image_height, ispc_cam *cam, int32_t num_triangles,
           ispc_triangle triangles[], int32_t num_lights, ispc_light lights[],
           int32_t num_light_triangles, ispc_triangle light_triangles[], float *return_image,
           int32_t debug, int32_t test);
#endif

/* ------------------------------------------------------------------------------------
 * Extended entry points (persistent device state, row bands, device-resident output)
 * ---------------------------------------------------------------------------------- */
typedef struct esc_context esc_context;

enum {
  ESC_FACE_FIXED = 0, /* faceID = fixed_face: the reference's behaviour for 1-face lights */
  ESC_FACE_HASH = 1   /* faceID = splitmix64(seed,pixel,light) % n_faces; replaces the
                         std::random_device-seeded mt19937 draw of main.cpp:587-588,743-747 */
};

enum {
  ESC_STAGE_AUTO = 0, /* fastest measured variant per pass */
  ESC_STAGE_SMEM = 1, /* primitives broadcast through the scalar cache into SGPRs */
  ESC_STAGE_LDS = 2,  /* primitives staged in LDS chunks by the workgroup: north_star's sketch, kept as
                         the REFERENCE-ARITHMETIC A/B PATH -- every (ray, primitive) pair runs the
                         reference's operations, no filters, no groups, no lists.  Not a performance
                         path: 20 % behind the scalar-cache staging when both ran that arithmetic
                         (round 1), one to two orders of magnitude behind the default today
                         (profiles/r03_final/stage_lds.txt).  What it is for: an independent
                         cross-check in the tests (same image, the reference's any-hit count). */
  ESC_STAGE_BVH = 3   /* opt-in acceleration structure (what the reference's --bvh flag meant to
                         be, main.cpp:98-171,331-415): screen-space bins for primary rays,
                         light-space bins for shadow rays and a bounding-volume tree behind both
                         cull primitives before the same exact tests run, so the image is the
                         brute-force image.  One kernel per frame.  Proven bounds
                         only: triangle meshes go through the default path's lists and groups
                         unless ESC_RENDER_BVH_HEURISTIC_PADS asks for the tree.
                         Never chosen by AUTO. */
};

typedef struct {
  int32_t shadows;   /* 1 = occlusion() evaluated (main.cpp:772); 0 = "primary rays only" */
  int32_t face_mode; /* ESC_FACE_* */
  int32_t fixed_face;
  int32_t stage; /* ESC_STAGE_* */
  uint64_t seed;
  int32_t pixels_per_lane; /* 0 = auto; 1, 2 or 4 pixels carried by each work-item of the primary
                              pass (same row, 16 columns apart).  Purely a scheduling choice:
                              results are bit-identical for every value.  Honoured by ESC_STAGE_LDS;
                              ESC_STAGE_SMEM / AUTO always carry 2 (the variant the packed filter
                              bodies are written for; the others spilled and were removed). */
  int32_t flags; /* ESC_RENDER_*; 0 = defaults */
} esc_render_options;

enum {
  /* Brute force evaluates a cheap conservative FILTER per (ray, sphere) and runs the reference
   * arithmetic only where the filter cannot rule a hit out (csrc/rt_brute.h "FILTERS"); the image
   * is the same bit for bit.  This flag (or $ESC_FILTER=0) runs the reference arithmetic for
   * every pair instead -- the round-1 kernels, kept as the A/B and as a cross-check in tests. */
  ESC_RENDER_EXACT_ONLY = 1,
  /* Record HIP events on the context's stream around and between the frame's two kernels
   * (k_primary, k_shade); esc_last_kernel_ms reads them.  Brute-force stages only: under
   * ESC_STAGE_BVH the frame is one kernel and ms[0] is 0. */
  ESC_RENDER_TIME_KERNELS = 2,
  /* The reference tests primitives in index order: closest hit with a strict `t2 < *t` (the lower
   * index keeps an equal t, main.cpp:176-192), occlusion() returning at the first hit
   * (main.cpp:314-329).  By default the brute-force kernels test in ANOTHER order wherever that
   * cannot be observed: from 64 spheres / 64 triangles up they sweep bounding spheres (and normal
   * cones) of spatial groups of 8 and open only the groups a ray of the wavefront may touch
   * (csrc/rt_device.h SphGroups / TriGroups) -- closest hits with the tie rule restated on the
   * original index; shadow rays of the LAST light stop at any occluder; shadow rays of earlier
   * lights, whose FIRST occluder in index order moves the next light's ray (quirk S3), visit
   * every group and keep the accepted primitive with the lowest original index.  Shorter sphere
   * lists of the last light are swept by decreasing solid angle.  Same image bit for bit, far fewer tests;
   * esc_counters.anyhit_tests then counts what THIS order executed.  This flag switches all of
   * that off: index order everywhere, anyhit_tests == the reference's count. */
  ESC_RENDER_INDEX_ORDER = 4,
  /* The shading pass has two forms with the same arithmetic: fused (one kernel, rays re-packed
   * inside each workgroup) and queue (one launch per segment of the primitive list, rays compacted
   * across the whole band).  By default the queue form is used for long lists (>= 2,048
   * primitives) on large bands (>= 1.5 M pixels) when the lists are swept linearly -- several
   * lights, or ESC_RENDER_INDEX_ORDER; a single light's grouped lists always take the fused form,
   * the only one that sweeps groups.  These force one. */
  ESC_RENDER_SHADE_QUEUE = 8,
  ESC_RENDER_SHADE_FUSED = 16,
  /* Primary rays of grouped tables do not sweep the group levels: per camera and band the library
   * lists, for every 32 x 4 pixel tile, the primitives its rays can touch (the projection of each
   * sphere grown by what the reference's rounding can reach, of each triangle dilated in its plane
   * by its bounding radius, plus the tiles a triangle's "nearly parallel" band crosses:
   * csrc/rt_lists.h), and a wavefront tests its tile's primitives directly.  Same filters and
   * reference arithmetic behind the lists, same image.  This flag (or $ESC_LISTS=0) keeps the
   * three-level sweep of round 2 for every tile -- the A/B switch and a cross-check in tests; tiles
   * whose lists overflow (more than 512 primitives) take that sweep anyway.  The lists cost 2 KB of
   * device memory per tile and primitive kind the scene has: 133 MB for a 4K frame, 531 MB at 8K. */
  ESC_RENDER_NO_TILE_LISTS = 32,
  /* The same from the light's end: a light that offers one sample point this frame (a one-face
   * light, or ESC_FACE_FIXED; the first 4 such lights) has all its shadow rays on lines through that
   * point, so the spheres / triangles a ray can reach are listed (as pair records) per direction cell
   * of a cube map around the point, once per scene and sample point (csrc/rt_lists.h "Light lists",
   * 25 MB per light and kind); a wavefront looks its rays' cells up and tests those lists -- inside
   * the wavefront, without the workgroup-wide re-packing of the sweeps, when every primitive kind of
   * the scene is covered.  This flag (or $ESC_LLISTS=0) keeps the three-level group sweep for every
   * shadow ray; rays the lists cannot serve (an overflowing cell, an origin outside the scene box)
   * take it anyway. */
  ESC_RENDER_NO_LIGHT_LISTS = 64,
  /* The default frame of the scalar-cache staging is ONE kernel (k_frame: closest hit and shading
   * of a 64 x 8 tile; no hit planes through HBM).  This flag (or $ESC_FRAME=2) keeps the two kernels
   * of rounds 1-2, k_primary + k_shade -- the A/B switch, and what ESC_RENDER_TIME_KERNELS and the
   * queue form of the shading pass use anyway.  Same arithmetic, same image. */
  ESC_RENDER_TWO_KERNELS = 128,
  /* ESC_STAGE_BVH culls with PROVEN bounds only: spheres through its tree and bins (box pads from
   * the error bound of the discriminant), triangle meshes (more than 4 triangles) through the tile /
   * light lists and group levels of the default path, whose reach statements cover the reference's
   * rounding-noise accepts for rays that graze a triangle's plane.  This flag sends triangle meshes
   * through the tree as well: its triangle boxes carry a HEURISTIC pad (2^-12 of the scene's
   * scale) -- faster on large meshes, every test and hunt so far bit-identical, but for rays within
   * ~1e-3 rad of a triangle's plane whose rounding-noise hit lies further than the pad outside the
   * triangle it may cull a hit the reference reports. */
  ESC_RENDER_BVH_HEURISTIC_PADS = 256,
  /* The ray counters (esc_counters: instrumentation the reference does not have) are not updated by
   * this call.  Counting costs two workgroup barriers, a handful of LDS and global atomics per
   * workgroup and a wave reduction per light and pixel: 9 % of a c4 frame.  Every frame of a fixed
   * scene, camera and option set counts the same rays, so a caller that wants both (bench.py) counts
   * one frame and times the others. */
  ESC_RENDER_NO_COUNTERS = 512,
  /* The shadow sweep reads the sphere light lists in a packed form derived from them: per cell only the
   * spheres whose own rectangle holds the cell, as copies of their constants, four per step (DESIGN.md
   * 3.9).  This flag makes it sweep the lists of pair-record ids instead, as before the packed form
   * existed -- the same image bit for bit, more tests: the A/B switch, and what the tests compare
   * against.  The lists themselves (esc_light_list_read) are the same either way. */
  ESC_RENDER_NO_PACKED_LIGHT_LISTS = 1024,
  /* When the host can prove that the light lists serve every shadow ray of a frame -- no cell or face
   * list over its cap, one light, a camera close enough to the scene that every shadow origin lies in
   * the box the lists were built for -- the one-kernel frame runs an instantiation
   * without the per-light workgroup vote and without the fallback sweep behind it.  This flag (or
   * $ESC_SURE=0) keeps the vote: the kernel every other frame runs anyway.  Same arithmetic, same
   * image; the A/B switch.  esc_last_frame_kernel tells which one ran. */
  ESC_RENDER_VOTE = 2048
};

/* esc_last_frame_kernel: the instantiation of the one-kernel frame (k_frame) the last frame launched */
enum {
  ESC_FRAME_KERNEL_FUSED = 1,  /* k_frame ran at all (0: two kernels, the queue form, another stage) */
  ESC_FRAME_KERNEL_GRP = 2,    /* primary rays through the groups / tile lists */
  ESC_FRAME_KERNEL_TGRP = 4,   /* the scene has triangle groups */
  ESC_FRAME_KERNEL_IDL = 8,    /* sphere light lists read by ids (or not at all), not in packed form */
  ESC_FRAME_KERNEL_SURE = 16   /* no vote, no fallback sweep (see ESC_RENDER_VOTE) */
};

typedef struct {
  uint64_t primary_rays; /* pixels rendered */
  uint64_t hit_pixels;   /* primary rays that hit something */
  uint64_t shadow_rays;  /* occlusion() calls (main.cpp:772): hit pixels x lights */
  uint64_t anyhit_tests; /* primitive tests those calls execute: up to and including the first
                            occluder met, else every primitive.  Equal to the reference's count
                            whenever the sweep is in index order (always with
                            ESC_RENDER_INDEX_ORDER; see there).  Group sweeps: per ray, the
                            super-group tests up to its occluder's (or all) plus 8 per group or
                            super-group opened on its behalf.  Under ESC_STAGE_BVH: the tests the
                            tree walk left for still-undecided rays */
  uint64_t anyhit_lane_tests; /* any-hit tests the GPU actually spent lanes on (64 per wave per
                                 primitive swept, decided or idle lanes included); the ratio
                                 anyhit_tests / anyhit_lane_tests is the lane efficiency of the
                                 shadow pass (SMEM stage only, 0 otherwise) */
} esc_counters;

/* Creates a context on HIP device `device` with its own stream.  Fails with
 * ESC_ERR_NO_DEVICE when there is no GPU: there is no CPU fallback. */
int esc_context_create(int32_t device, esc_context **out);
void esc_context_destroy(esc_context *ctx);
/* Launch on the caller's hipStream_t instead (e.g. a torch stream's handle). */
int esc_context_set_stream(esc_context *ctx, void *hip_stream);
/* Process-wide: how many device buffers the contexts of this library hold right now, and their bytes
 * (either pointer may be NULL).  Destroying a context gives back everything it allocated. */
int esc_live_device_allocations(int64_t *buffers, int64_t *bytes);
void *esc_context_stream(esc_context *ctx);
int esc_context_synchronize(esc_context *ctx);

/* == flatten + hipMemcpy: stages the scene as SoA tables in HBM (replaces
 * flatten_scene_ispc's role at main.cpp:591-605).  Re-upload replaces the previous one. */
int esc_upload_scene(esc_context *ctx, const esc_scene *scene);
/* same, from ISPC flat arrays (what trace() does internally) */
int esc_upload_flat(esc_context *ctx, int32_t num_triangles, const ispc_triangle *triangles,
                    int32_t num_lights, const ispc_light *lights, int32_t num_light_triangles,
                    const ispc_triangle *light_triangles);

/* Host-only check of the arrays `trace` / esc_upload_flat would stage (no GPU needed): geom ids
 * >= 0, every light with >= 1 face and a non-null light_faces whose entries index
 * light_triangles[].  It cannot detect a DANGLING light_faces pointer -- the reference's own
 * flatten_scene_ispc leaves one (flatten_iscp.cpp:39,103); use esc_flatten_ispc instead. */
int esc_check_flat(int32_t num_triangles, const ispc_triangle *triangles, int32_t num_lights,
                   const ispc_light *lights, int32_t num_light_triangles,
                   const ispc_triangle *light_triangles);

/* == the row loop main.cpp:628-636 restricted to rows [row_begin,row_end) of a W x H frame
 * (scan_row, main.cpp:28-30, is the row-granular seam).  Asynchronous on the context's
 * stream.  Outputs are DEVICE pointers, band-local: pixel (w,h) at ((h-row_begin)*W+w)*3.
 *   d_rgb_f32  fp32 RGB accumulators (may be NULL)
 *   d_rgb_u8   8-bit RGB after the PPM clamp/truncate of main.cpp:676-682 (may be NULL)
 * Device pointers must be 4-byte aligned (d_rgb_u8 excepted: any address); a misaligned d_rgb_f32 is
 * ESC_ERR_INVALID and nothing is launched.  Exactly the band's (row_end - row_begin) * W * 3 elements
 * of each non-NULL output are written, every pixel of the band, misses (0, 0, 0) included, and nothing
 * else; an empty band writes nothing.
 * Counters accumulate on the device; read them with esc_read_counters (synchronises). */
int esc_render_rows(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                    int32_t row_begin, int32_t row_end, const esc_render_options *opts,
                    float *d_rgb_f32, uint8_t *d_rgb_u8);
/* Multi-GPU partition: the image is cut into strips of `strip_rows` rows counted from h = 0
 * (strip k = rows [k*strip_rows, (k+1)*strip_rows), the last one possibly short); this call
 * renders strips first_strip, first_strip + strip_stride, ... -- i.e. rank r of N calls it
 * with (first_strip = r, strip_stride = N).  Dealing strips round-robin balances sky rows
 * (primary rays only) against floor rows (primary + shadow).  strip_rows must be a multiple of
 * 8.  Output: the rendered rows packed in ascending h, esc_strip_local_rows() of them: exactly those
 * rows * W * 3 elements of each non-NULL output are written (none when the rank has no strip).
 * Alignment as for esc_render_rows: d_rgb_f32 4-byte aligned or ESC_ERR_INVALID, d_rgb_u8 anywhere. */
int esc_render_strips(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                      int32_t strip_rows, int32_t first_strip, int32_t strip_stride,
                      const esc_render_options *opts, float *d_rgb_f32, uint8_t *d_rgb_u8);
/* number of rows the call above renders (>= 0), or ESC_ERR_INVALID */
int esc_strip_local_rows(int32_t H, int32_t strip_rows, int32_t first_strip,
                         int32_t strip_stride);
/* A recorded frame: the launches of one esc_render_strips call captured into a HIP graph, replayed
 * with ONE host call per frame.  At 8 GPUs a rank's share of a 4K frame is a few tens of
 * microseconds of GPU work, the same order as the host side of a plain frame (parameter block, two
 * or more kernel launches); a recorded frame costs one hipGraphLaunch.  esc_frame_record renders one
 * plain frame first (it builds everything the kernels read), then captures the second.  A recorded
 * frame replays exactly those launches -- same camera, band, options and output buffers -- and is
 * only valid while the context's per-camera / per-scene device state stands: esc_frame_launch
 * returns ESC_ERR_INVALID once the context has rendered another camera, size or scene, or had a
 * scene uploaded, or has freed or reallocated any buffer a frame kernel reads or writes (record
 * again).  Counters accumulate as for plain frames.  ESC_RENDER_TIME_KERNELS cannot be recorded.
 * Outputs and alignment as for esc_render_strips, checked before anything is launched or captured: a
 * misaligned d_rgb_f32 is ESC_ERR_INVALID, *out is not written, and frames recorded earlier stay valid.
 * Every esc_frame_launch writes the same elements again and nothing else. */
typedef struct esc_frame esc_frame;
int esc_frame_record(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t strip_rows,
                     int32_t first_strip, int32_t strip_stride, const esc_render_options *opts,
                     float *d_rgb_f32, uint8_t *d_rgb_u8, esc_frame **out);
int esc_frame_launch(esc_frame *frame); /* asynchronous, on the context's stream */
/* 1 when esc_frame_launch would accept the frame (the same comparison), 0 when it would refuse it or
 * frame is NULL. */
int esc_frame_valid(const esc_frame *frame);
void esc_frame_destroy(esc_frame *frame);

/* After a gather of N such buffers to one device (block r at d_gathered + r*rank_pitch_bytes):
 * writes the H x W frame in (h*W+w) order.  bytes_per_pixel = 12 (fp32 RGB) or 3 (u8 RGB).
 * Exactly H * W * bytes_per_pixel bytes of d_frame are written; of a rank's block only its local rows
 * are read, so padding behind them (rank_pitch_bytes larger than the block) never reaches the frame;
 * d_gathered is not modified and must not overlap d_frame.  With a pixel size that is a multiple of 4
 * bytes both device pointers must be 4-byte aligned (ESC_ERR_INVALID, nothing launched); byte pixels
 * may sit at any address.  Asynchronous on the context's stream. */
int esc_assemble_strips(esc_context *ctx, const void *d_gathered, int32_t n_ranks,
                        size_t rank_pitch_bytes, int32_t W, int32_t H, int32_t strip_rows,
                        int32_t bytes_per_pixel, void *d_frame);
/* ---- acceleration structure (ESC_STAGE_BVH) -------------------------------------------
 * Built on the host from the uploaded scene the first time a frame asks for ESC_STAGE_BVH (or by
 * esc_build_accel), rebuilt when the camera leaves the region its conservative box pads were
 * computed for.  The reference times its tree build apart from the render as well
 * (main.cpp:569-579). */
typedef struct { /* 64 bytes; boxes of both children live in the parent */
  float lo0[3], hi0[3];
  float lo1[3], hi1[3];
  int32_t child[2];   /* >= 0 node index; < 0 leaf: ~block */
  uint32_t minkey[2]; /* smallest primitive key (triangles, then spheres) below each child */
} esc_bvh_node;
typedef struct {
  int32_t tri_nodes, tri_blocks, tri_depth, tri_root; /* blocks of 2 triangles */
  int32_t sph_nodes, sph_blocks, sph_depth, sph_root; /* blocks of 4 spheres */
  float build_ms; /* host build + upload, last build */
  int32_t builds; /* how many times this context has built */
  int32_t reserved[2];
} esc_accel_info;
int esc_build_accel(esc_context *ctx, const float origin[3]);
int esc_get_accel_info(esc_context *ctx, esc_accel_info *out);
/* Host only (no GPU): the same builder over a scene, for inspection and tests.  which = 0
 * triangles, 1 spheres.  Any output pointer may be NULL; counts come back in `info`.
 * prim_boxes receives the padded box of every primitive (lo xyz, hi xyz). */
int esc_scene_build_accel(const esc_scene *scene, const float origin[3], int32_t which,
                          esc_accel_info *info, esc_bvh_node *nodes, int64_t nodes_cap,
                          int32_t *order, int64_t order_cap, float *prim_boxes,
                          int64_t prim_boxes_cap);

/* The per-scene tables of a scene upload, in the record layouts of csrc/rt_device.h: first the
 * staged scene, then what the host computes from it for the brute-force kernels (pair tables, the
 * shadow filters' forms, the last light's sweep order, sphere and triangle groups: empty where the
 * scene is below that table's threshold), then one esc_scene_table_header. */
enum {
  ESC_TABLE_TRI = 0,      /* DevTri */
  ESC_TABLE_TRI_N,        /* DevTriN; empty when no geometry has normals */
  ESC_TABLE_SPH,          /* DevSph */
  ESC_TABLE_SPH_MAT,      /* int32 material index per sphere */
  ESC_TABLE_MAT,          /* DevMat: geometries, then spheres */
  ESC_TABLE_TRANSMIT,     /* 4 floats per material: tf[3], ni */
  ESC_TABLE_LIGHTS,       /* DevLight */
  ESC_TABLE_LIGHT_POINTS, /* 4 floats per sample point: xyz0 */
  ESC_TABLE_SPH2,         /* DevSphPair */
  ESC_TABLE_SPH2_F,       /* DevSphPairF */
  ESC_TABLE_SPH2_ORD,     /* DevSphPair, the last light's sweep order */
  ESC_TABLE_SPH2_F_ORD,   /* DevSphPairF, same order */
  ESC_TABLE_TRI2_F,       /* DevTriPairF */
  ESC_TABLE_TRI2_PF,      /* DevTriPairPF */
  ESC_TABLE_SG_SORTED,    /* SphGroups: DevSph */
  ESC_TABLE_SG_GRP,       /* DevSphGroup: groups, super-groups, hyper-groups */
  ESC_TABLE_SG_ORIG,      /* DevIdx4 */
  ESC_TABLE_SG_SORTED2,   /* DevSphPair */
  ESC_TABLE_SG_SORTED2_F, /* DevSphPairF */
  ESC_TABLE_SG_GRP2_F,    /* DevSphPairF */
  ESC_TABLE_TG_SORTED,    /* TriGroups: DevTri */
  ESC_TABLE_TG_GRP,       /* DevTriGroup: groups, super-groups, hyper-groups */
  ESC_TABLE_TG_ORIG,      /* DevIdx4 */
  ESC_TABLE_TG_SORTED2_F, /* DevTriPairF */
  ESC_TABLE_TG_SORTED2_PF, /* DevTriPairPF */
  ESC_TABLE_TG_GRP2_PF,   /* DevTriPairPF */
  ESC_TABLE_HEADER,       /* esc_scene_table_header */
  ESC_TABLE_COUNT
};
typedef struct {     /* 72 bytes */
  float g[3];        /* the scene point the shadow filters work around (middle of the scene box) */
  float rho_max;     /* shadow-ray origins further than this (1-norm) from g take the exact path */
  float scene_lo[3]; /* the scene box grown by 5 %, rounded outwards (light lists) */
  float scene_hi[3];
  int32_t sg_n_grp, sg_n_sup, sg_n_hyp; /* sphere groups, super-groups, hyper-groups (pads included) */
  int32_t tg_n_grp, tg_n_sup, tg_n_hyp; /* the same for triangles */
  int32_t any_transmissive;             /* 1 when some material has tf > 0 and ni > 0 */
  int32_t min_light_faces;              /* smallest face count among the lights; 0 without lights */
} esc_scene_table_header;
/* Host only (no GPU), for inspection and tests: table `which` (ESC_TABLE_*) of the tables
 * esc_upload_scene computes for this scene, as the bytes it uploads.  Returns the table's size in
 * bytes (copied when capacity suffices; out may be NULL to ask for the size) or a negative error. */
int64_t esc_scene_table(const esc_scene *scene, int32_t which, void *out, int64_t capacity);

/* Host only: the segments the queue form of the shading pass cuts occlusion()'s primitive list
 * into (main.cpp:314-329 order: triangles, then spheres).  segments receives 4 ints per segment:
 * first triangle, triangle count, first sphere PAIR record, pair-record count (either count may
 * be 0).  Returns the number of segments (<= capacity) or a negative error.  For inspection and
 * tests: every primitive must be covered exactly once, in order. */
int esc_queue_schedule(int32_t n_triangles, int32_t n_spheres, int32_t *segments,
                       int32_t capacity);

/* Host only, for inspection and tests: the static record of `count` triangles taken as ONE group
 * of the brute-force kernels' triangle groups (csrc/rt_device.h DevTriGroup): v0e1e2 holds 9
 * floats per triangle (vert0, vert1 - vert0, vert2 - vert0); record receives 12 floats:
 * centre xyz, rgeo, cone axis xyz, smax, rext, b0, b1, always.  Returns 0 or a negative error. */
int esc_tri_group_record(const float *v0e1e2, int32_t count, float record[12]);

/* The same for spheres (csrc/rt_device.h DevSphGroup): cxyzr2 holds 4 floats per sphere (centre,
 * r^2); record receives centre xyz and rgeo >= r_i + |c_i - centre| for every sphere. */
int esc_sphere_group_record(const float *cxyzr2, int32_t count, float record[4]);

/* Host only, for inspection and tests: the geometry behind the tile lists of the primary pass
 * (csrc/rt_tile_math.h, the code the binning kernels run).  esc_tile_rect: the pixel rectangle
 * rect = {w0, w1, h0, h1} (inclusive, clipped to the image) outside which no primary ray's line
 * passes within `radius` of `centre`; returns 1 (rectangle), 2 (wholly off screen), 0 (unbounded:
 * the camera plane cuts the sphere -- such a group is tested by every tile) or a negative error.
 * esc_tile_band: 1 when some ray of the pixels [32 tile_x, 32 tile_x + 32) x [row, row + 4) may
 * have |d . normal| <= kp (`normal` a unit vector, d the reference's unit direction), else 0. */
int esc_tile_rect(const esc_camera *cam, int32_t W, int32_t H, const float centre[3], double radius,
                  int32_t rect[4]);
int esc_tile_band(const esc_camera *cam, int32_t W, int32_t H, int32_t tile_x, int32_t row,
                  const float normal[3], double kp);

/* For inspection and tests: the tile lists the last frame of this context was rendered with
 * (which = 0 spheres, 1 triangles; 2 = the light lists of the shadow pass: one "tile" per direction
 * cell, tiles_x = cells per face side, tile_rows = faces x cells per side, hdr[0] = the longest
 * face-global list).  hdr receives {global primitives, cone entries, lists-off
 * flag, tiles_x, tile_rows, list capacity, global capacity, 0}; counts (may be NULL) the appended
 * primitive count of up to `capacity` tiles -- a count above the list capacity means that tile took
 * the three-level sweep.  Returns the number of tiles, 0 when the context holds no lists, or a
 * negative error.  Synchronises the context's stream. */
int esc_tile_list_counts(esc_context *ctx, int32_t which, int32_t hdr[8], int32_t *counts,
                         size_t capacity);

/* ... and the entries of ONE tile / cell (`index` in the order of esc_tile_list_counts): slots of
 * the group-sorted tables (which = 0, 1) or pair records (2, 3).  Returns the appended count (the
 * list holds min(count, capacity of the list) entries; at most `capacity` are copied).
 * index = -1 with which = 0 or 1: the GLOBAL list of that kind, the slots every tile tests (returns the
 * appended count hdr[0]; min(count, global capacity, `capacity`) entries are copied).  The light lists
 * (2, 3) keep one global list per face and have no such call: index = -1 is ESC_ERR_INVALID there. */
int esc_tile_list_ids(esc_context *ctx, int32_t which, int64_t index, int32_t *ids, int32_t capacity);

/* The per-tile triangle masks of the last frame, for inspection and tests; read-only.  A scene whose
 * triangle table is swept directly (no groups, so esc_tile_list_counts(which = 1) reports no lists) and
 * holds 1 to 32 triangles gets one 32-bit word per 32 x 4 pixel tile of the band: bit k set means some
 * primary ray of the tile may be accepted by triangle k (original index).  info receives {state, global
 * word, tiles per row, tile rows, triangles, 0, 0, 0}: state != 0 -- the masks switched themselves off for
 * this camera and every tile tests every triangle; the global word's triangles are tested by every tile.
 * Up to `capacity` words are copied to `masks` (may be NULL), tiles in the order of esc_tile_list_counts.
 * Returns the number of tiles, 0 when the last frame had no masks (more than 32 triangles or none, a
 * grouped table, a band that does not start on a multiple of 4 rows, pixels_per_lane 1 or 4,
 * ESC_RENDER_NO_TILE_LISTS and the other paths that take no lists), or a negative error.  Synchronises the context's stream. */
int esc_tile_tri_masks(esc_context *ctx, int32_t info[8], uint32_t *masks, size_t capacity);

/* ... and the light lists (which = 2 sphere pair records, 3 triangle pair records) as a whole, for
 * inspection and tests; read-only.  info receives {lights with lists, cells per face side R, list
 * capacity, global capacity, point[0..3]}: point[li] is the row of the light_points table the lists of
 * light li were built for.  Cells are numbered ((light * 6 + face) * R + cw) * R + cu, the order of
 * esc_tile_list_counts.  Each of the three outputs may be NULL:
 *   face_counts [lights * 6]                    the appended count of every (light, face) list;
 *   face_ids    [lights * 6][global capacity]   its stored ids, min(count, global capacity) of them, then -1;
 *   cell_ids    [n_cells][list capacity]        the stored ids of cells first_cell .. first_cell + n_cells - 1,
 *                                               min(count, list capacity) of each, then -1 -- one copy
 *                                               for the whole range.
 * Returns the number of cells of all lists, 0 when the context holds no light lists of that kind (nothing
 * is written then), or a negative error (a range that leaves the lists: ESC_ERR_INVALID).  Synchronises
 * the context's stream. */
int esc_light_list_read(esc_context *ctx, int32_t which, int32_t info[8], int32_t *face_counts,
                        int32_t *face_ids, int64_t first_cell, int64_t n_cells, int32_t *cell_ids);

/* ... and the packed form of the sphere light lists (csrc/rt_device.h LightLists::pk_*), the form the
 * shadow sweep reads.  info receives {lights with lists, R, slots per cell in `slots` (2 * list capacity),
 * spheres per step (4), steps of all cells, 0, 0, 0}.  Either output may be NULL:
 *   steps [n_cells]                     the cell's step count; -1: the cell is over its list capacity and
 *                                       is not served (the sweep runs instead);
 *   slots [n_cells][2 * list capacity]  the cell's 4 * steps slots in the order they are tested, each the
 *                                       position 2 j + h of a sphere in the group-sorted table (half h of
 *                                       pair record j) or -1 for a pad slot; -1 after them.
 * Returns as esc_light_list_read does; 0 also when the valid lists have no packed form. */
int esc_light_list_packed_read(esc_context *ctx, int32_t info[8], int64_t first_cell, int64_t n_cells,
                               int32_t *steps, int32_t *slots);

/* Host only, for inspection and tests: the spatial order the groups are cut from (k-d median
 * splits over the points; csrc/rt_device.h SphGroups / TriGroups).  xyz holds 3 floats per point;
 * order receives a permutation of 0 .. count-1 whose consecutive runs of `run`, `big` and `huge`
 * points (each a multiple of the one before) are subtrees of the splits. */
int esc_group_order(const float *xyz, int32_t count, int32_t run, int32_t big, int32_t huge,
                    int32_t *order);
/* ms[0] = k_primary, ms[1] = k_shade of the last frame rendered with ESC_RENDER_TIME_KERNELS
 * (waits for that frame).  This is how bench.py prices each kernel against its own roof. */
int esc_last_kernel_ms(esc_context *ctx, float ms[2]);
/* ESC_FRAME_KERNEL_* bits of the last frame this context launched (esc_render_rows / esc_render_strips /
 * esc_frame_record; a recorded frame keeps the kernel it was recorded with), or a negative error. */
int esc_last_frame_kernel(esc_context *ctx);
/* Reads and clears the word k_frame's ESC_FRAME_KERNEL_SURE instantiation sets when a wavefront was
 * refused by the light lists after all -- which the launch conditions rule out: a check for tests, 0
 * always.  Returns 0 or 1, or a negative error.  Synchronises the context's stream. */
int esc_frame_tripwire(esc_context *ctx);
/* A check for tests: the exact tail of the triangle test takes 1 / det (ray_triangle.h:26, det a widened
 * float) from a reciprocal refined by hand instead of the compiler's f64 division.  Runs that helper on
 * the device over the float bit patterns first_bits .. first_bits + n - 1 (modulo 2^32; n <= 2^32) and
 * compares it, as 64-bit integers, with 1.0 / (double)x wherever x passes the range test in front of it
 * (ray_triangle.h:23-25: every |x| >= FLT_EPSILON, the infinities and the NaNs).  *mismatches receives
 * the number of patterns that differ, *first_mismatch the smallest of them (0 when there is none).
 * Synchronises the context's stream. */
int esc_check_inv_det_exact(esc_context *ctx, uint32_t first_bits, uint64_t n, uint64_t *mismatches,
                            uint32_t *first_mismatch);
/* Host only: 1 when every shadow-ray origin fl(origin + dir (t - eps)) of a camera at `origin` -- any
 * direction, any primary hit the kernels accept in `scene` -- lies inside the scene's grown box
 * (esc_scene_table_header scene_lo / scene_hi), by the sufficient condition of DESIGN.md 3.9; 0 when the
 * condition does not hold (a camera too far away, or nearly in the plane of a triangle, a scene with more
 * than one light, a non-finite coordinate); a negative error. */
int esc_scene_shadow_origins_inside(const esc_scene *scene, const float origin[3]);
int esc_reset_counters(esc_context *ctx);
int esc_read_counters(esc_context *ctx, esc_counters *out);

/* ---- batched ray queries ---------------------------------------------------------------
 * The reference's two primitive loops on rays of the caller's own (picking, visibility or
 * ambient-occlusion baking, collision probes, custom shading passes).  Every pointer is a DEVICE
 * pointer, 4-byte aligned; the calls are asynchronous on the context's stream; n == 0 launches
 * nothing (and the pointers may then be NULL).  A query reads only the uploaded scene's tables: no
 * camera state, tile or light lists, render counters or recorded frame is touched.
 * Results are bit-identical to the reference arithmetic for any float input (non-unit, zero, NaN
 * or infinite directions, origins anywhere): a ray that is not unit to a few ulp, starts outside
 * the region the culling bounds were proven for, or has a NaN bound runs the reference loop itself
 * (counted in esc_query_stats.exact_rays).
 * flags: 0, or ESC_RENDER_EXACT_ONLY (every pair through the reference arithmetic in index order,
 * no filters, no groups: the A/B and the tests' reference on large scenes); other bits are
 * rejected. */
typedef struct {
  uint64_t rays;        /* rays of the last query call */
  uint64_t exact_rays;  /* rays that took the exact sweep (all of them under ESC_RENDER_EXACT_ONLY) */
  uint64_t exact_tests; /* (ray, primitive) pairs that ran the reference arithmetic */
} esc_query_stats;
/* Closest hit == intersect() / cpp_intersect() (main.cpp:176-192, 302-312): per ray, t starts at
 * d_tmax[i] (NULL: FLT_MAX, main.cpp:715) and intersect_triangle (ray_triangle.h:7-57) runs over
 * every triangle, geometry by geometry and face by face, then the sphere extension over every
 * sphere (after every triangle in tie order).  Outputs: d_t[i] (== the bound on a miss),
 * d_geom[i] / d_prim[i] = geometry index and face index of a triangle hit (for a scene uploaded
 * with esc_upload_flat: the triangle's geom_id and its index in triangles[]), -1 / k for sphere k,
 * -1 / -1 for a miss; d_uv (n x 2, may be NULL) = the u2, v2 intersect_triangle writes for the
 * winning triangle (quirk S1 is the caller's aliasing, main.cpp:307-310, not the function's),
 * 0 / 0 otherwise.  d_origins, d_dirs: n x 3 floats. */
int esc_intersect_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                       const float *d_tmax, float *d_t, int32_t *d_geom, int32_t *d_prim,
                       float *d_uv, uint32_t flags);
/* Occlusion == occlusion() (main.cpp:314-329) with the sphere extension: d_occluded[i] = 1 if any
 * primitive is accepted with t carried from d_tmax[i] (NULL: FLT_MAX), else 0 -- the same answer
 * as "esc_intersect_rays found a hit". */
int esc_occluded_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      const float *d_tmax, uint8_t *d_occluded, uint32_t flags);
/* counts of the last query call on this context (zero before the first); synchronises the
 * context's stream */
int esc_last_query_stats(esc_context *ctx, esc_query_stats *out);

/* ---- shading of caller-supplied rays, camera rays, supersampled frames ----------------------
 * scan_row's body (main.cpp:698-791) on rays the caller supplies: any camera model, several samples
 * per pixel.  Same conventions as the queries above: DEVICE pointers, 4-byte aligned (byte outputs
 * excepted), asynchronous on the context's stream, n == 0 launches nothing, only the uploaded scene's
 * tables are read (no camera state, tile or light lists, render counters or recorded frame), and the
 * results are bit-identical to the reference arithmetic for any float input.
 *
 * Primary rays of the frame as data == camera.h:31-34 get_ray as main.cpp:709-713 calls it: ray
 * i = (h - row_begin)*W + w of rows [row_begin, row_end) has origin cam.origin and direction
 * normalize(((llc + horizontal*s) + vertical*t) - origin), s = (float(w) + dx) / float(W-1),
 * t = (float(h) + dy) / float(H-1), (dx, dy) = d_offsets[2i], d_offsets[2i+1] in pixels (NULL: 0).
 * With no offsets these are, bit for bit, the rays esc_render_rows traces.  d_origins, d_dirs: n x 3
 * floats, n = (row_end - row_begin)*W.  Needs W,H >= 2. */
int esc_camera_rays(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t row_begin,
                    int32_t row_end, const float *d_offsets, float *d_origins, float *d_dirs);
/* counts of the last esc_shade_rays / esc_render_supersampled call (a NEW struct: esc_query_stats
 * keeps its layout) */
typedef struct {
  uint64_t rays;        /* rays shaded */
  uint64_t hit_rays;    /* rays whose closest hit found a primitive (main.cpp:722) */
  uint64_t shadow_rays; /* occlusion() calls (main.cpp:772; 0 when shadows == 0) */
  uint64_t exact_rays;  /* primary or shadow rays that took the index-order reference loop */
  uint64_t exact_tests; /* (ray, primitive) pairs that ran the reference arithmetic */
} esc_shade_stats;
/* main.cpp:698-791 for each ray (o, d) = (d_origins[i], d_dirs[i]), n x 3 floats each:
 *   - closest hit with t from FLT_MAX (main.cpp:715-722): d_t, d_geom, d_prim (each NULL or n) equal
 *     esc_intersect_rays on the same ray;
 *   - the normal (main.cpp:723-738): face normal, then vertex normals with u == 0 (quirk S1); spheres
 *     normalize((o + d*t) - C) with the ray's own o;
 *   - per light in order (main.cpp:740-789): the light sample of quirk S2 (face fixed_face under
 *     ESC_FACE_FIXED, face_hash(seed, pixel_base + i mod 2^32, light, n_faces) under ESC_FACE_HASH),
 *     hit = o + d*(t - FLT_EPSILON), t = len - FLT_EPSILON, occlusion() with that t -- the occluder
 *     of the lowest index, whose t2 the next light starts from (quirk S3) -- and Phong.
 * d_rgb (n x 3, required) receives the colour, d_rgb8 (n x 3 bytes, or NULL) the PPM quantisation of
 * main.cpp:676-682.  opts: shadows (0 = primary only), face_mode, fixed_face, seed and flags (0 or
 * ESC_RENDER_EXACT_ONLY: every primary and shadow ray through the reference loop in index order);
 * stage must be ESC_STAGE_AUTO, other flags are rejected, pixels_per_lane is ignored.  A primary or
 * shadow ray outside the filters' preconditions (see the queries above) runs the reference loop. */
int esc_shade_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t pixel_base,
                   const esc_render_options *opts, float *d_rgb, uint8_t *d_rgb8, float *d_t, int32_t *d_geom,
                   int32_t *d_prim);
/* synchronises the context's stream */
int esc_last_shade_stats(esc_context *ctx, esc_shade_stats *out);
/* Anti-aliased frame: spp = n*n samples per pixel (n in 1..8) on a regular grid.  Sample k = j*n + i
 * is the frame's ray through (w + dx, h + dy), dx = (i + 0.5f)/n - 0.5f, dy = (j + 0.5f)/n - 0.5f
 * (fp32), shaded by esc_shade_rays with pixel index h*W + w and seed opts.seed + k.  Per pixel and
 * channel acc = 0; acc += rgb_k for k = 0 .. spp-1 (fp32, in that order); d_image = acc / float(spp)
 * and d_u8 (or NULL) = its quantisation (main.cpp:676-682).  spp == 1 is esc_render_rows over the
 * whole frame, bit for bit.  d_image: W*H*3 floats, the layout of esc_render_rows.  Works in bands of
 * rows with at most 256 MB of scratch.  Asynchronous. */
int esc_render_supersampled(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                            const esc_render_options *opts, float *d_image, uint8_t *d_u8);

/* ---- adaptive supersampling: refine only the pixels on an edge (rt_adaptive.hip, DESIGN.md section
 * 3.16) ----
 * An anti-aliased frame that pays the spp samples only where the 1-sample frame has contrast.  All
 * comparisons are fp32:
 *   1. B = the frame esc_render_rows writes for rows [0, H) with `opts`, bit for bit, on the frame
 *      kernels (as a render call it touches camera state, lists and render counters the way
 *      esc_render_rows does);
 *   2. M[h,w] = 1 iff some 4-neighbour (h',w') inside the frame and some channel c has
 *      !(fabsf(B[h,w,c] - B[h',w',c]) <= threshold): a NaN difference refines, both pixels of an edge
 *      pair refine, and M is defined on the whole of B, never on pixels that were already refined;
 *   3. a pixel with M = 1 takes the value esc_render_supersampled(spp) gives that pixel, bit for bit
 *      (sample k = j*n + i at (i + 0.5f)/n - 0.5f, (j + 0.5f)/n - 0.5f, pixel id h*W + w, seed
 *      opts.seed + k, acc = 0; acc += rgb_k in order; acc / float(spp));
 *   4. every other pixel keeps B.
 * d_image: W*H*3 floats; d_u8 (or NULL) the quantisation of the final image (main.cpp:676-682); d_mask
 * (W*H bytes, or NULL) receives M.  spp == 1, or a threshold nothing exceeds, gives the frame itself, bit
 * for bit.  Asynchronous on the context's stream: the masked pixels are listed and refined on the device,
 * no host synchronisation happens inside the call.  The scratch is the context's and only grows: 1 byte
 * per pixel for M when d_mask is NULL, plus 4 bytes per pixel of a band for the list; band_rows == 0
 * keeps the list at or below 256 MB.  The image does not depend on band_rows.
 * spp, W, H, cam, opts and alignment follow esc_render_supersampled; a negative, NaN or infinite
 * threshold, reserved != 0 or band_rows < 0 is ESC_ERR_INVALID. */
typedef struct esc_adaptive_options {
  int32_t spp;       /* n*n, n in 1..8: samples of a refined pixel */
  float threshold;   /* >= 0, finite */
  int32_t band_rows; /* 0 = automatic; > 0: refine in bands of this many rows (memory knob) */
  int32_t reserved;  /* 0 */
} esc_adaptive_options;
/* counts of the last esc_render_adaptive call (zero before the first) */
typedef struct esc_adaptive_stats {
  uint64_t pixels;         /* W * H */
  uint64_t refined_pixels; /* pixels with M = 1 */
  uint64_t samples;        /* refined_pixels * spp */
  /* of the refinement rays, as esc_shade_stats counts them */
  uint64_t hit_rays;
  uint64_t shadow_rays;
  uint64_t exact_rays;
  uint64_t exact_tests;
} esc_adaptive_stats;
int esc_render_adaptive(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                        const esc_render_options *opts, const esc_adaptive_options *adaptive_opts,
                        float *d_image, uint8_t *d_u8, uint8_t *d_mask);
/* synchronises the context's stream */
int esc_last_adaptive_stats(esc_context *ctx, esc_adaptive_stats *out);

/* ---- mirror reflections: a fused on-device bounce loop (rt_trace.hip) ----
 * An extension beyond the reference (which casts no secondary rays), driven by the material's ks.
 * For one ray (o, d) with pixel id q = pixel_base + i (mod 2^32), max_depth = D and bias, all
 * arithmetic fp32, one rounding per written operation, no contraction, vec.h's operation order for
 * dot, normalize, vector +- and vector * scalar:
 *
 *   w = (1, 1, 1)
 *   for k = 0 .. D:
 *       (c, t0, id, N) = what esc_shade_rays computes for (o, d) with pixel id q and seed
 *                        opts.seed + 64*k (mod 2^64): c the colour; t0 the closest-hit t of
 *                        main.cpp:715-722 (NOT the t the light loop carries, quirk S3); N the shading
 *                        normal of main.cpp:723-738 incl. quirk S1, spheres normalize((o + d*t0) - C)
 *       C = c                       if k == 0
 *       C = C + w * c               otherwise, per channel: fl(C + fl(w * c))
 *       stop if id is a miss or k == D
 *       w = w * ks(material of id)  per channel
 *       stop unless (w.r > 0 || w.g > 0 || w.b > 0)      (a NaN or zero weight ends the path)
 *       s  = dot(d, N)
 *       Nf = (s > 0) ? -N : N
 *       o' = (o + d * t0) + Nf * bias
 *       d' = normalize(d - N * (2.f * s))
 *       (o, d) = (o', d')
 *   result C, and its PPM quantisation (main.cpp:676-682) in d_rgb8
 *
 * A supersampled frame's sample j at depth k uses seed + j + 64*k (j < 64).  A bounce ray is an
 * ordinary ray to the sweeps: it passes the precondition gate of the queries or runs the reference
 * loop in index order.  With bias == 0 a bounce may hit its own surface again at t ~ 0; that is
 * defined behaviour (the reference's shadow rays have the same property) and bias is the remedy.
 * max_depth == 0 is esc_shade_rays, bit for bit (while the context holds no environment: see
 * esc_set_environment, which gives the rays that miss a colour at every level, level 0 included).
 *
 * Pointer, alignment, n == 0, flag and stage rules are esc_shade_rays'; ESC_RENDER_EXACT_ONLY sends
 * every primary, bounce and shadow ray through the index-order loop.  max_depth outside 0..16 or a
 * negative / NaN / infinite bias is ESC_ERR_INVALID.  Asynchronous on the context's stream: one
 * launch per depth level, no host synchronisation between them; the ray queues live in scratch the
 * context owns (rays are processed in batches so that it stays under 256 MB).  Like the queries the
 * calls read only per-scene tables. */
#define ESC_TRACE_MAX_DEPTH 16
/* counts of the last esc_trace_rays / esc_render_traced call (a NEW struct: the others keep their
 * layout).  rays counts every shaded ray, primary and bounce: the sum of depth_rays. */
typedef struct esc_trace_stats {
  uint64_t rays;
  uint64_t hit_rays;
  uint64_t shadow_rays;
  uint64_t exact_rays;  /* primary, bounce and shadow rays that ran the index-order loop */
  uint64_t exact_tests;
  uint64_t depth_rays[ESC_TRACE_MAX_DEPTH + 1]; /* rays shaded at each level */
} esc_trace_stats;
int esc_trace_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t pixel_base,
                   const esc_render_options *opts, int32_t max_depth, float bias, float *d_rgb, uint8_t *d_rgb8);
/* camera rays -> the loop above -> the accumulate / finish of esc_render_supersampled (same spp
 * rules, sample offsets and pixel ids), in row bands under the 256 MB scratch cap, queues included.
 * max_depth == 0 is esc_render_supersampled, bit for bit (while the context holds no environment). */
int esc_render_traced(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                      int32_t max_depth, float bias, const esc_render_options *opts, float *d_image,
                      uint8_t *d_u8);
/* synchronises the context's stream */
int esc_last_trace_stats(esc_context *ctx, esc_trace_stats *out);

/* ---- refraction: transmitted rays through glass and water (rt_trace.hip, rt_transmit.h, DESIGN.md
 * section 3.14) ----
 * The loop of esc_trace_rays with one more way of computing the next ray at a hit whose material has
 * a transmission entry (esc_scene_set_geometry_transmission, esc_upload_scene; esc_upload_flat
 * carries none: all opaque).  One ray per hit: a transmissive surface either refracts or reflects, so
 * the queue bound and the plain update of C hold as before.  With T = (tf, ni) the table entry of the
 * hit's material, q the ray's pixel id and seed_k the level's seed (opts.seed (+ j) + 64*k), the step
 * after "stop if id is a miss or k == D" reads, with the same arithmetic rules as above:
 *
 *   transmissive = mode != OFF && (tf.r > 0 || tf.g > 0 || tf.b > 0) && ni > 0        (NaN: false)
 *   if !transmissive:   the rule of esc_trace_rays (w = w * ks, stop unless some w > 0, mirror bounce)
 *   else:
 *       s   = dot(d, N);   Nf = (s > 0) ? -N : N;   c1 = (s > 0) ? s : -s
 *       eta = (s > 0) ? ni : 1.f / ni                      (s > 0: the ray leaves the medium)
 *       k   = 1.f - (eta * eta) * (1.f - c1 * c1)
 *       reflect = !(k >= 0)                      (total internal reflection; also a NaN k)  -> total_internal
 *       if !reflect && mode == FRESNEL:
 *           r0 = (ni - 1.f) / (ni + 1.f);  r0 = r0 * r0
 *           cx = (s > 0) ? sqrt(k) : c1                    (the cosine on the outside of the surface)
 *           m  = 1.f - cx;   m2 = m * m;   F = r0 + (1.f - r0) * ((m2 * m2) * m)
 *           u  = float(mix(seed_k, q, 0xFFFFFFFF) >> 8) * 2^-24
 *           reflect = u < F                                                           -> fresnel_reflected
 *       if reflect:   o' = (o + d * t0) + Nf * bias;   d' = normalize(d - N * (2.f * s))     (w unchanged)
 *       else:         w = w * tf;  stop unless (w.r > 0 || w.g > 0 || w.b > 0)              -> refracted
 *                     o' = (o + d * t0) - Nf * bias;   d' = normalize(d * eta + Nf * (eta * c1 - sqrt(k)))
 *
 * mix(seed, pixel, light) is the 64-bit mixer of the light-face hash (splitmix64's finaliser over
 * seed + (pixel << 32 | light) + 0x9E3779B97F4A7C15), its high 32 bits before the modulo; no light has
 * index 0xFFFFFFFF, so the choice is independent of the light-face choice.  The material's own colour
 * c is still added at the hit; the ks of a transmissive material drives no bounce.  The medium
 * outside every surface has index 1 (no nested media).  SHADOW RAYS ARE UNCHANGED: a transmissive
 * primitive occludes like any other (the reference's occlusion loop).  With FRESNEL the two branches
 * mix over the samples of esc_render_traced_ex (sample j has its own seed); REFRACT is the noise-free
 * choice at spp 1.  esc_transmit_stats counts the rays each arrow above sent on to the next level
 * (a refracted ray whose weight ends the path is not counted), so that with the mirror bounces they
 * add up to depth_rays of the following levels.
 *
 * ESC_TRANSMIT_OFF is esc_trace_rays / esc_render_traced, bit for bit, and so is any mode on a scene
 * without a transmissive entry.  transmission outside 0..2 or reserved != 0 is ESC_ERR_INVALID; the
 * other argument rules are esc_trace_rays'.  esc_last_trace_stats works after these calls too. */
#define ESC_TRANSMIT_OFF 0     /* esc_trace_rays, bit for bit */
#define ESC_TRANSMIT_REFRACT 1 /* a transmissive surface refracts; total internal reflection reflects */
#define ESC_TRANSMIT_FRESNEL 2 /* Schlick's F decides, by a hash of (seed, pixel, level), between the two */
typedef struct esc_trace_options {
  int32_t max_depth;
  float bias;
  int32_t transmission; /* ESC_TRANSMIT_* */
  int32_t reserved;     /* 0 */
} esc_trace_options;
int esc_trace_rays_ex(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      uint32_t pixel_base, const esc_render_options *opts, const esc_trace_options *trace_opts,
                      float *d_rgb, uint8_t *d_rgb8);
int esc_render_traced_ex(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                         const esc_render_options *opts, const esc_trace_options *trace_opts, float *d_image,
                         uint8_t *d_u8);
/* counts of the last esc_trace_rays_ex / esc_render_traced_ex call (zero after the plain forms) */
typedef struct esc_transmit_stats {
  uint64_t refracted;
  uint64_t fresnel_reflected;
  uint64_t total_internal;
} esc_transmit_stats;
/* synchronises the context's stream, like esc_last_trace_stats */
int esc_last_transmit_stats(esc_context *ctx, esc_transmit_stats *out);

/* ---- ambient occlusion: hemisphere visibility of rays and frames (rt_ambient.hip, DESIGN.md section
 * 3.17) ----
 * An extension beyond the reference, whose ambient term is the constant ka * 0.5: how many of K directions
 * of the hemisphere above a ray's hit point are open within a radius.  The result is an integer count per
 * ray.  All arithmetic is fp32 with one rounding per written operation, no contraction, vec.h's operation
 * order for dot, normalize, vector +- and vector * scalar, and consists of + - * / and sqrt only: the
 * sample directions are DATA, a table the caller supplies.
 *
 * The table: S sets x K samples x 3 floats (1 <= S, K <= 64), local directions about +z, row-major
 * (table[set][k] at 3*(set*K + k)).  Its contents are never validated.  esc_set_ambient_table copies it
 * from HOST memory to the device; it belongs to the context and survives scene uploads (a new table
 * replaces it).  esc_ambient_cosine_table fills one on the host, without a context, with cosine-weighted
 * unit vectors (z > 0): deterministic in (sets, samples, seed), drawn with the host's libm -- the result
 * is data that a caller can read back, store or replace.
 *
 * For ray i with origin o and direction d (used as given), K = opts.samples, S = opts.sets (the first K
 * samples of the first S sets of the context's table: each at most the table's own):
 *
 *   1. (t, id) = the closest hit esc_intersect_rays finds with bound FLT_MAX.  A miss: count = K.
 *   2. N = the normal esc_shade_rays computes (main.cpp:723-738 incl. quirk S1, u = 0; a sphere:
 *      normalize((o + d*t) - C))
 *   3. sn = dot(d, N);  Nf = (sn > 0) ? -N : N;  P = (o + d*t) + Nf*bias         (esc_trace_rays' bounce origin)
 *   4. sg = copysign(1, Nf.z);  a = -1 / (sg + Nf.z);  b = (Nf.x*Nf.y)*a          (|sg + Nf.z| >= 1)
 *      T = (1 + (sg*(Nf.x*Nf.x))*a,  sg*b,  -(sg*Nf.x))
 *      B = (b,  sg + (Nf.y*Nf.y)*a,  -Nf.y)
 *   5. set = mix(opts.seed, pixel_base + i mod 2^32, 0xFFFFFFFE) mod S            (mix: see esc_trace_options;
 *      no light has index 0xFFFFFFFE and the Fresnel draw uses 0xFFFFFFFF, so the three draws are independent)
 *   6. for k = 0 .. K-1:  l = table[set][k];  w = normalize((T*l.x + B*l.y) + Nf*l.z)
 *      sample k is open iff esc_occluded_rays(P, w, tmax = radius) is 0;  count = the open samples
 *   7. vis = float(count) / float(K)                                              (a miss: 1.0f)
 *
 * A sample ray is an ordinary ray to the sweeps: the reference's normalize() leaves w within precondition
 * (c) of the filtered sweep, and a ray outside the preconditions runs the reference loop in index order.
 * With bias == 0 a sample may meet its own surface at t ~ 0, decided by the reference's own rounding
 * (esc_trace_rays says the same of its bounces); bias is the remedy.
 *
 * radius: finite and > 0, FLT_MAX = unbounded.  bias: finite and >= 0.  flags: 0 or ESC_RENDER_EXACT_ONLY
 * (every primary and sample ray through the index-order loop).  Anything else, samples or sets outside
 * 1 .. the table's, or a call before esc_set_ambient_table is ESC_ERR_INVALID.  Pointer, alignment and
 * n == 0 rules are esc_shade_rays'; the calls are asynchronous on the context's stream and read only
 * per-scene tables and the sample table. */
typedef struct esc_ambient_options {
  int32_t samples;     /* K */
  int32_t sets;        /* S */
  float radius;
  float bias;
  uint64_t seed;
  uint32_t pixel_base; /* esc_ambient_rays: the hash's pixel of ray 0; esc_render_ambient ignores it */
  uint32_t flags;
} esc_ambient_options;
/* counts of the last esc_ambient_rays / esc_render_ambient / esc_skylight_rays / esc_render_skylight call
 * (zero before the first): the sky lighting calls run the same primary and sample rays and report the same
 * six counters */
typedef struct esc_ambient_stats {
  uint64_t rays;
  uint64_t hit_rays;         /* rays whose closest hit found a primitive */
  uint64_t samples;          /* sample rays: K * hit_rays */
  uint64_t occluded_samples; /* sample rays that met a primitive within the radius */
  uint64_t exact_rays;       /* primary or sample rays that took the index-order reference loop */
  uint64_t exact_tests;      /* (ray, primitive) pairs that ran the reference arithmetic */
} esc_ambient_stats;
/* host_table: sets * samples * 3 floats in HOST memory; synchronises the context's stream */
int esc_set_ambient_table(esc_context *ctx, int32_t sets, int32_t samples, const float *host_table);
/* out: sets * samples * 3 floats in host memory; needs no context and no device */
int esc_ambient_cosine_table(int32_t sets, int32_t samples, uint64_t seed, float *out);
/* d_vis (n floats, required) receives vis; d_count (n int32), d_t, d_geom, d_prim (each NULL or n) the
 * count and what esc_intersect_rays gives for the same ray */
int esc_ambient_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                     const esc_ambient_options *opts, float *d_vis, int32_t *d_count, float *d_t,
                     int32_t *d_geom, int32_t *d_prim);
/* ray i = h*W + w is ray i of esc_camera_rays(cam, W, H, 0, H, NULL), made inside the kernel, with pixel id
 * i (pixel_base 0): bit for bit esc_ambient_rays on those rays.  d_vis: W*H floats, d_count: W*H or NULL.
 * W, H and cam follow esc_render_supersampled. */
int esc_render_ambient(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                       const esc_ambient_options *opts, float *d_vis, int32_t *d_count);
/* d_out[3i + c] = fl(d_rgb[3i + c] * d_vis[i]) for n pixels, and d_out8 = its quantisation
 * (main.cpp:676-682).  d_out may be d_rgb itself; d_out or d_out8 may be NULL, not both.  Asynchronous. */
int esc_modulate(esc_context *ctx, int64_t n, const float *d_rgb, const float *d_vis, float *d_out,
                 uint8_t *d_out8);
/* synchronises the context's stream; reports esc_skylight_rays / esc_render_skylight too */
int esc_last_ambient_stats(esc_context *ctx, esc_ambient_stats *out);

/* ---- sky lighting: the open ambient samples gather the environment (rt_ambient.hip, DESIGN.md section
 * 3.19) ----
 * The environment cube (esc_set_environment, below) as a diffuse light: the cosine-weighted mean of env(w_k)
 * over the open samples of ambient occlusion is the diffuse irradiance estimator, image-based ambient
 * lighting with contact shadows.  It adds no random draw and no device transcendental to what
 * esc_ambient_rays and env(d) already consist of: + - * /, sqrt and the lookup's floor.
 *
 * Steps 1-7 of esc_ambient_options are unchanged: they give the hit, N, Nf, P, T, B, the set, the w_k, and
 * open / occluded against radius, count and vis.  Then, all in fp32 with one rounding per written operation:
 *
 *   8. s = (+0, +0, +0).  for k = 0 .. K-1, in this order: if sample k is open:
 *          e = env(w_k)   (env(d) of esc_set_environment on the context's cube, w_k exactly as step 6 made it)
 *          s_c = fl(s_c + e_c)  for c = r, g, b
 *      An occluded sample adds nothing.
 *      sky_c = fl(s_c / float(K)).  A miss: sky = (0, 0, 0), with count = K and vis = 1 as before.
 *   9. light_c = fl(kd_c * sky_c), kd of the hit's material (material floats 3..5; a sphere's through its
 *      material index).  A miss: light = (0, 0, 0).
 *
 * A miss carries no light on purpose: traced frames already show the sky there, and frame + light must not
 * add it twice.  The estimator divides by K, not by the open count: the samples are cosine-weighted, so sky
 * is irradiance / pi and kd * sky is the diffuse radiance.  With an all-ones cube sky == vis in every
 * channel, bit for bit.
 *
 * opts is esc_ambient_options, unchanged, with its rules.  The calls need both a sample table and an
 * environment: a call without either is ESC_ERR_INVALID with a message naming it.  Validation, alignment,
 * n == 0 and asynchrony follow esc_ambient_rays and esc_modulate.  vis, count, t, geom and prim are those of
 * esc_ambient_rays with the same options, bit for bit, and esc_last_ambient_stats reports these calls too.
 * Out of scope: the environment as a light for esc_shade_rays, frames or the bounce loop, specular or glossy
 * reflection of the sky, importance sampling of bright texels, bounce light. */
/* d_sky, d_light: n x 3 floats each, either may be NULL, not both; d_vis (n floats), d_count (n int32), d_t,
 * d_geom, d_prim: each NULL or n, as esc_ambient_rays writes them */
int esc_skylight_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      const esc_ambient_options *opts, float *d_sky, float *d_light, float *d_vis,
                      int32_t *d_count, float *d_t, int32_t *d_geom, int32_t *d_prim);
/* the rays of esc_render_ambient, made inside the kernel: bit for bit esc_skylight_rays on
 * esc_camera_rays(cam, W, H, 0, H, NULL) with pixel_base 0.  d_sky, d_light: W*H*3 floats, either may be
 * NULL, not both; d_vis: W*H floats or NULL; d_count: W*H or NULL. */
int esc_render_skylight(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                        const esc_ambient_options *opts, float *d_sky, float *d_light, float *d_vis,
                        int32_t *d_count);
/* d_out[3i + c] = fl(d_rgb[3i + c] + d_light[3i + c]) for n pixels, and d_out8 = its quantisation
 * (main.cpp:676-682).  d_out may be d_rgb itself; d_out or d_out8 may be NULL, not both.  Asynchronous. */
int esc_add_light(esc_context *ctx, int64_t n, const float *d_rgb, const float *d_light, float *d_out,
                  uint8_t *d_out8);

/* ---- G-buffer of rays and frames, and the edge-stopping a-trous filter it guides (rt_gbuffer.hip,
 * rt_filter.hip) ----
 * Ambient occlusion and sky lighting estimate every pixel from K <= 64 samples drawn by a hash, so vis, sky
 * and light are banded or noisy.  The filter averages such an image over neighbouring pixels of the same
 * surface; which neighbours those are is decided by per-pixel guides: the shading normal, the hit position
 * and the surface's id.  The G-buffer calls hand the guides out.
 *
 * The G-buffer, per ray (o, d).  All arithmetic is fp32 with one rounding per operation, in vec.h's order,
 * exactly as steps 1-2 of esc_ambient_options:
 *
 *   (t, id)  = the closest hit esc_intersect_rays finds with bound FLT_MAX; t, geom, prim are its outputs
 *   normal   = the normal esc_shade_rays computes (main.cpp:723-738 incl. quirk S1, u = 0; a sphere:
 *              normalize((o + d*t) - C)).  It is NOT flipped towards the ray.
 *   position = fl(o + fl(d*t))
 *   albedo   = kd of the hit's material (material floats 3..5; a sphere's through its material index)
 *   a miss:    normal = position = albedo = (+0, +0, +0), t = FLT_MAX, geom = prim = -1
 *
 * Each of the six outputs may be NULL, not all of them (when n > 0).  flags: 0 or ESC_RENDER_EXACT_ONLY (every
 * ray through the index-order loop).  Pointer, alignment, n == 0 and asynchrony rules are esc_ambient_rays'; only
 * per-scene tables are read, and no sample table or environment is needed.  t, geom and prim are
 * byte-identical to what esc_ambient_rays and esc_intersect_rays write for the same rays. */
typedef struct esc_gbuffer_stats {
  uint64_t rays;
  uint64_t hit_rays;    /* rays whose closest hit found a primitive */
  uint64_t exact_rays;  /* rays that took the index-order reference loop */
  uint64_t exact_tests; /* (ray, primitive) pairs that ran the reference arithmetic */
} esc_gbuffer_stats;
/* d_normal, d_position, d_albedo: n x 3 floats each; d_t: n floats; d_geom, d_prim: n int32 */
int esc_gbuffer_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t flags,
                     float *d_normal, float *d_position, float *d_albedo, float *d_t, int32_t *d_geom,
                     int32_t *d_prim);
/* ray i = h*W + w is ray i of esc_camera_rays(cam, W, H, 0, H, NULL), made inside the kernel: bit for bit
 * esc_gbuffer_rays on those rays.  The outputs hold W*H rays.  W, H and cam follow esc_render_ambient. */
int esc_render_gbuffer(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, uint32_t flags,
                       float *d_normal, float *d_position, float *d_albedo, float *d_t, int32_t *d_geom,
                       int32_t *d_prim);
/* counts of the last esc_gbuffer_rays / esc_render_gbuffer call (zero before the first); synchronises the
 * context's stream */
int esc_last_gbuffer_stats(esc_context *ctx, esc_gbuffer_stats *out);

/* The filter: L iterations of a 5 x 5 a-trous (with holes) B3-spline kernel whose taps are accepted or
 * rejected by COMPARES on the guides and weighted by the kernel's dyadic constants alone.  It consists of
 * + - * / and compares: the usual exp() edge weights are deliberately not used, because no transcendental
 * may run on the device, and so the result is comparable bit for bit.
 *
 * Images are interleaved (channels = 1 or 3 floats per pixel) and pixel (w, h) is at h*W + w, in the image
 * and in the four guide arrays (d_normal, d_position: W*H x 3 floats; d_geom, d_prim: W*H int32, as
 * esc_render_gbuffer writes them).  With
 *
 *   hit(p)    = geom[p] >= 0 || prim[p] >= 0
 *   K1        = (1/16, 1/4, 3/8, 1/4, 1/16)
 *   k(dx, dy) = K1[dx+2] * K1[dy+2]                                      (exact in fp32)
 *
 * I_0 = in, and for i = 0 .. L-1 with s = 1 << i, I_{i+1} at pixel p = (w, h) is, all in fp32 with one
 * rounding per written operation:
 *
 *   if !hit(p):  I_{i+1}[p] = I_i[p]                                     (copied, bit for bit)
 *   else:  acc_c = +0 for every channel;  ws = +0
 *     for dy = -2 .. 2 (ascending), inside it dx = -2 .. 2 (ascending):
 *        q = (w + dx*s, h + dy*s);   skip unless 0 <= q.w < W and 0 <= q.h < H     (no clamping, no mirroring)
 *        if (dx, dy) != (0, 0):                                                    -> taps_tested += 1
 *           skip unless hit(q)
 *           skip if same_object and !(geom[q] == geom[p] && (geom[p] >= 0 || prim[q] == prim[p]))
 *           skip unless dot(N_p, N_q) >= normal_cos                  (vec.h dot: sum = 0; sum += a_i*b_i)
 *           skip unless fabsf(dot(P_q - P_p, N_p)) <= plane_dist     (the difference per component first)
 *                                                                                  -> taps_accepted += 1
 *        acc_c = fl(acc_c + fl(k(dx,dy) * I_i[q]_c));   ws = fl(ws + k(dx,dy))
 *     I_{i+1}[p]_c = fl(acc_c / ws)
 *   out = I_L
 *
 * The centre tap is never tested, so ws >= 9/64, and a pixel with NaN guides still gets fl(fl(k0*v)/k0).
 * A comparison with a NaN guide is false, so that tap is skipped.  A NaN or infinite image value spreads to
 * whatever accepts it, as written.  "same object" is the same geometry for triangles and the same sphere
 * for spheres.  The stats are summed over the L iterations; pixels = W*H and hit_pixels are counted once.
 *
 * d_out must not be d_in (ESC_ERR_INVALID), so no iteration reads what it writes: the iterations alternate
 * between d_out and one context-owned scratch image so that the last one lands in d_out (L odd:
 * in -> out -> S -> out ...; L even: in -> S -> out ...).  Scratch, owned by the context, grow-only and
 * freed with it: 32 bytes per pixel for the packed guides (N.xyz, geom, P.xyz, prim), and for L >= 2 one
 * image of 4 * channels bytes per pixel.  Growing it waits for the context's stream; otherwise the call is
 * asynchronous on the stream with no host synchronisation.  It needs no scene.
 * ESC_ERR_INVALID: iterations outside 1..8, channels other than 1 or 3, a NaN threshold, a negative
 * plane_dist, same_object other than 0 / 1, a non-zero reserved, W or H < 1, a null or misaligned pointer.
 * Out of scope: variance-guided weights, any smooth weight, albedo demodulation.  Accumulation over frames is
 * esc_temporal_accumulate, below. */
typedef struct esc_filter_options {
  int32_t iterations;  /* L, 1..8: iteration i uses step 2^i pixels */
  float normal_cos;    /* a tap needs dot(N_p, N_q) >= normal_cos; not NaN */
  float plane_dist;    /* ... and |dot(P_q - P_p, N_p)| <= plane_dist; >= 0, not NaN; FLT_MAX or inf: off */
  int32_t same_object; /* 0 / 1: ... and the same geometry (triangles) or the same sphere */
  int32_t reserved[2]; /* 0 */
} esc_filter_options;
typedef struct esc_filter_stats {
  uint64_t pixels;        /* W*H */
  uint64_t hit_pixels;    /* pixels with hit(p): the others are copied */
  uint64_t taps_tested;   /* non-centre taps inside the image of hit pixels, over all iterations */
  uint64_t taps_accepted; /* ... that passed every stop */
} esc_filter_stats;
int esc_filter_guided(esc_context *ctx, int32_t W, int32_t H, int32_t channels, const float *d_in,
                      const float *d_normal, const float *d_position, const int32_t *d_geom, const int32_t *d_prim,
                      const esc_filter_options *opts, float *d_out);
/* counts of the last esc_filter_guided call (zero before the first); synchronises the context's stream */
int esc_last_filter_stats(esc_context *ctx, esc_filter_stats *out);

/* ---- temporal accumulation: reproject ambient and sky light from the previous frame (rt_temporal.hip,
 * DESIGN.md section 3.21) ----
 * The filter above spreads a frame's K samples per pixel over space; this call keeps them over time.  Every hit
 * pixel's world-space point is looked up in the previous frame: where the previous camera saw that point, and
 * whether it is still the same surface there.  If so, the new estimate is blended into what was accumulated,
 * so a caller with a moving camera can run few samples per frame with a new seed each frame, and a still
 * camera refines progressively.  It consists of + - * /, floorf and compares: no transcendental, and the
 * history taps are accepted or rejected by the filter's hard compares, so the result is comparable bit for bit.
 *
 * Images are interleaved (channels = 1 or 3 floats per pixel) and pixel (w, h) is at h*W + w, in the images,
 * in d_history_n / d_out_n and in the guide arrays.  cur holds the guides of the frame that produced
 * d_current; prev, d_history and d_history_n belong to the previous frame, rendered with prev_cam at the same
 * W x H.  The current camera is not needed: position is a world-space point.  hit(.) is the filter's,
 * geom >= 0 || prim >= 0.  All arithmetic is fp32 with one rounding per written operation; dot, cross and the
 * vector + - * are in vec.h's operation order.  With M = max_history, for pixel p = (w, h):
 *
 *   if !hit_cur(p):  out[p] = current[p] (copied, bit for bit);  out_n[p] = 0
 *   else:
 *     A = prev_cam.lower_left_corner - prev_cam.origin;   Hh = prev_cam.horizontal;   V = prev_cam.vertical
 *     v = P_p - prev_cam.origin                                   (per component)
 *     c   = cross(V, v);          det = dot(Hh, c)
 *     x   = dot(A, c) / det;      y = dot(Hh, cross(A, v)) / det;      z = dot(Hh, cross(V, A)) / det
 *           (x Hh + y V + z v = A: the previous camera's ray through s = -x, t = -y passes through P_p,
 *            in front of the camera iff z > 0)
 *     fx  = (-x) * float(W - 1);  fy = (-y) * float(H - 1)        (the inverse of s = w/(W-1), t = h/(H-1))
 *     valid = z > 0 && fx >= -1.f && fx <= float(W) && fy >= -1.f && fy <= float(H)      (a NaN anywhere: false)
 *     acc_c = +0;  ws = +0;  n = INT32_MAX
 *     if valid:
 *       taps == 1:  x0 = floorf(fx + 0.5f);  y0 = floorf(fy + 0.5f);  one tap (i, j) = (0, 0) with k = 1.f
 *       taps == 4:  x0 = floorf(fx);  ax = fx - x0;  y0 = floorf(fy);  ay = fy - y0
 *                   taps (j, i) = (0,0), (0,1), (1,0), (1,1) in this order,
 *                   k = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay)
 *       for each tap:  q = (x0 + i, y0 + j)
 *         skip unless 0 <= q.w <= W-1 and 0 <= q.h <= H-1       (compared as floats BEFORE any conversion to int)
 *         skip unless k > 0                                                                 -> taps_tested += 1
 *         skip unless hit_prev(q)
 *         skip unless history_n[q] >= 1
 *         skip if same_object and !(geom_prev[q] == geom_cur[p] && (geom_cur[p] >= 0 || prim_prev[q] == prim_cur[p]))
 *         skip unless dot(N_p, Nprev_q) >= normal_cos
 *         skip unless fabsf(dot(Pprev_q - P_p, N_p)) <= plane_dist                          -> taps_accepted += 1
 *         acc_c = fl(acc_c + fl(k * history[q]_c));   ws = fl(ws + k);   n = min(n, history_n[q])
 *     if !(ws > 0):  out[p] = current[p];  out_n[p] = 1
 *     else:                                                                                 -> reused_pixels += 1
 *       m = min(n, M - 1) + 1;   alpha = 1.f / float(m)
 *       hc = fl(acc_c / ws);     out[p]_c = fl(hc + fl(fl(current[p]_c - hc) * alpha));   out_n[p] = m
 *
 * What follows from it:
 *   - A first frame is this call with d_history_n all zero: every tap is refused, the output is current, and
 *     n = 1 on hits.
 *   - A pixel's n is the smallest n among its accepted taps, plus one, capped at M.  Up to M the value is the
 *     running mean; from M on it is an exponential average with alpha = 1/M.
 *   - Pixels without a hit carry no history (n = 0).
 *   - The scene is assumed static between the two frames, because positions are compared in world space.  The
 *     object, normal and plane stops are what reject disocclusions; nothing detects a moved object.
 *   - A comparison with a NaN is false: a NaN position or camera makes the pixel not valid, a NaN guide skips
 *     the tap.  A NaN or infinite history or current value spreads to the pixels that accept it, as written.
 *
 * d_out must not be d_history and d_out_n must not be d_history_n (ESC_ERR_INVALID each), because taps read
 * neighbours; d_out may be d_current.  ESC_ERR_INVALID also: W or H < 2, channels other than 1 or 3, taps
 * other than 1 or 4, max_history outside 1..65536, a NaN threshold, a negative plane_dist, same_object other
 * than 0 / 1, a non-zero reserved, a null or misaligned (4 bytes) pointer.  The call is asynchronous on the
 * context's stream with no host synchronisation, needs no scene and no scratch; the stats counters are device
 * words the context owns and frees.
 * Out of scope: motion vectors for moving objects, variance or moment buffers, colour-box clamping, albedo
 * demodulation, reprojecting specular or traced colour. */
typedef struct esc_guides {          /* four arrays as esc_render_gbuffer writes them, W*H pixels, DEVICE pointers */
  const float *normal;               /* W*H x 3 */
  const float *position;             /* W*H x 3 */
  const int32_t *geom, *prim;        /* W*H each */
} esc_guides;
typedef struct esc_temporal_options {
  int32_t taps;         /* 1: the nearest history pixel; 4: bilinear over the 2 x 2 around the reprojected point */
  int32_t max_history;  /* M, 1..65536: the history length saturates at M (alpha never below 1/M) */
  float normal_cos;     /* as esc_filter_options; not NaN */
  float plane_dist;     /* as esc_filter_options; >= 0, not NaN; FLT_MAX or inf: off */
  int32_t same_object;  /* 0 / 1 */
  int32_t reserved[3];  /* 0 */
} esc_temporal_options;
typedef struct esc_temporal_stats {
  uint64_t pixels;        /* W*H */
  uint64_t hit_pixels;    /* pixels with hit_cur(p): the others are copied */
  uint64_t reused_pixels; /* hit pixels that accepted at least one history tap (ws > 0) */
  uint64_t taps_tested;   /* taps inside the previous image with k > 0 */
  uint64_t taps_accepted; /* ... that passed every stop */
} esc_temporal_stats;
int esc_temporal_accumulate(esc_context *ctx, const esc_camera *prev_cam, int32_t W, int32_t H, int32_t channels,
                            const float *d_current, const esc_guides *cur,
                            const float *d_history, const int32_t *d_history_n, const esc_guides *prev,
                            const esc_temporal_options *opts, float *d_out, int32_t *d_out_n);
/* counts of the last esc_temporal_accumulate call (zero before the first); synchronises the stream */
int esc_last_temporal_stats(esc_context *ctx, esc_temporal_stats *out);

/* ---- environment cube map: traced rays that miss see a sky (rt_environ.h, rt_environ.hip, rt_trace.hip,
 * DESIGN.md section 3.18) ----
 * An extension beyond the reference, whose framebuffer is black where nothing is hit.  The texels are DATA
 * the caller supplies, like the ambient table; the lookup consists of + - * /, floor and compares only, so
 * it is comparable bit for bit: a cube map and not a latitude / longitude map, no atan2 / acos runs anywhere.
 *
 * The cube: R texels per side, 1 <= R <= ESC_ENV_MAX_RES.  Host layout texels[face][j][i][3] floats,
 * row-major (texel (face, j, i) at 3*((face*R + j)*R + i)); face order +x, -x, +y, -y, +z, -z, so
 * face = 2*axis + (negative ? 1 : 0).  Its contents are never validated.
 *
 * The lookup env(d) for a direction d, used as given (it need not be of unit length).  All arithmetic fp32,
 * one rounding per written operation, no contraction:
 *
 *   ax = |d.x|, ay = |d.y|, az = |d.z|
 *   axis = 0 if (ax >= ay && ax >= az) else 1 if (ay >= az) else 2        (comparisons with NaN are false)
 *   m = |d[axis]|;  a = d[(axis+1) % 3];  b = d[(axis+2) % 3];  negative = d[axis] < 0
 *   env(d) = (0, 0, 0)  unless no component of d is NaN and 0 < m <= FLT_MAX
 *   u = a / m;  v = b / m                                         (both in [-1, 1]; no mirroring per face)
 *   x = ((u * 0.5f + 0.5f) * float(R)) - 0.5f;   x0 = floorf(x);  fx = x - x0
 *   i0 = clamp(int(x0), 0, R-1);  i1 = clamp(int(x0) + 1, 0, R-1)       (the same for y from v: j0, j1, fy)
 *   per channel, t = the face's texels:
 *       c0 = t[j0][i0] + (t[j0][i1] - t[j0][i0]) * fx
 *       c1 = t[j1][i0] + (t[j1][i1] - t[j1][i0]) * fx
 *       env = c0 + (c1 - c0) * fy
 *
 * Bilinear inside a face and clamped at the face border; NO filtering across faces: a discontinuity of up
 * to half a texel's gradient at a seam is the documented price.  R == 1 is one colour per face.  A constant
 * cube returns its colour exactly.  x lies in [-0.5, R - 0.5] and fx in [0, 1]: fx rounds to 1 only for an x
 * just under 0, where both indices are clamped to 0.
 *
 * The rule in the bounce loop (esc_trace_rays, esc_trace_rays_ex, esc_render_traced, esc_render_traced_ex):
 * while the context holds an environment, at EVERY level k the line "(c, t0, id, N) = what esc_shade_rays
 * computes" is followed by
 *
 *       if id is a miss: c = env(d)
 *
 * and everything else is unchanged: C = c at level 0, C = fl(C + fl(w * c)) afterwards, and "stop if id is
 * a miss" still ends the path.  The environment emits nothing onto surfaces, is invisible to shadow rays
 * and does not change which rays bounce: depth_rays, hit_rays and esc_transmit_stats are those of the same
 * call without an environment.  Without an environment every call launches the kernels it always launched.
 * UNCHANGED, with black where nothing is hit: esc_render_rows and everything built on the frame kernels,
 * esc_shade_rays, esc_render_supersampled, esc_render_adaptive, the queries and ambient occlusion.
 * The environment as a diffuse light source is esc_skylight_rays (above).
 * Out of scope: coloured shadows, latitude / longitude maps and image loaders, filtering across faces, mip
 * levels, a per-call switch (clear the environment instead). */
#define ESC_ENV_MAX_RES 1024 /* the device copy holds 16 bytes per texel: 100 MB at 1024 */
/* host_texels: 6*res*res*3 floats in HOST memory, copied (and repacked) to the device.  The environment
 * belongs to the context and survives scene uploads; a new one replaces it; res == 0 with host_texels ==
 * NULL removes it.  Synchronises the context's stream before and after.  res outside 0..1024, or exactly
 * one of the two arguments being empty, is ESC_ERR_INVALID. */
int esc_set_environment(esc_context *ctx, int32_t res, const float *host_texels);
/* *res = R of the context's environment, 0 when none is set */
int esc_get_environment_res(esc_context *ctx, int32_t *res);
/* A vertical gradient as a cube, on the host, without a context or a device.  out: 6*res*res*3 floats.
 * Texel (face, j, i) stands for D with D[axis] = +-1, D[(axis+1)%3] = ((i + 0.5)/R)*2 - 1,
 * D[(axis+2)%3] = ((j + 0.5)/R)*2 - 1;  e = D.y / sqrt((D.x*D.x + D.y*D.y) + D.z*D.z);  the colour is
 * horizon + (zenith - horizon)*e for e >= 0, otherwise horizon + (ground - horizon)*(-e): all in double in
 * that operation order, then cast to float.  No libm transcendental takes part.  The result is data a
 * caller can read, store or replace.  res outside 1..1024 or a null pointer is ESC_ERR_INVALID. */
int esc_environment_sky(int32_t res, const float zenith[3], const float horizon[3], const float ground[3],
                        float *out);
/* env(d) for n directions of the caller's own (background plates; the lookup without tracing), and its PPM
 * quantisation (main.cpp:676-682).  DEVICE pointers: d_dirs n*3 floats, d_rgb n*3 floats, d_rgb8 n*3
 * bytes; either output may be NULL, not both.  Asynchronous on the context's stream; n == 0 launches
 * nothing.  Needs an environment (else ESC_ERR_INVALID) but no scene. */
int esc_environment_rays(esc_context *ctx, int64_t n, const float *d_dirs, float *d_rgb, uint8_t *d_rgb8);
/* The same lookup on the host, for inspection and tests: the very code the kernels run (rt_environ.h),
 * compiled for the host.  texels in the host layout above, dirs and rgb n*3 floats in host memory. */
int esc_environment_lookup_host(int32_t res, const float *texels, int64_t n, const float *dirs, float *rgb);

/* ---- thin-lens camera: depth of field for camera rays and traced frames (rt_lens.h, rt_lens.hip,
 * DESIGN.md section 3.22) ----
 * An extension beyond the reference, whose camera.h:31-34 sends every ray of a pixel through one point.  Here
 * a ray starts at a point of a lens disk of radius `aperture` about the camera's origin and aims at the point
 * where the pinhole ray meets the plane at distance `focus_dist` along the view axis: that plane stays sharp,
 * everything nearer or farther blurs.  The points of the disk are DATA the caller supplies (the lens table),
 * like the ambient table; the device runs no transcendental and the rule is comparable bit for bit.
 *
 * The lens table: S sets x K samples x 2 floats, 1 <= S, K <= 64, points (x, y) of the unit disk, row-major:
 * table[set][k] at 2*(set*K + k).  Its contents are never validated.
 *
 * All arithmetic is fp32, one rounding per written operation, no contraction; normalize, vector +- and
 * vector x scalar in vec.h's operation order; only + - * / and sqrt.  The ray of pixel (w, h) with sub-pixel
 * offset (dx, dy), lens sample index k and pixel id q = h*W + w:
 *
 *   is = (float(w) + dx) / float(W-1);   it = (float(h) + dy) / float(H-1)
 *   p  = ((llc + horizontal*is) + vertical*it) - origin
 *   if aperture == 0:   o' = origin;  d' = normalize(p)                      (esc_camera_rays' statements)
 *   else:
 *       U   = normalize(horizontal);   V = normalize(vertical)
 *       set = mix(lens.seed, q, 0xFFFFFFFD) mod S
 *             (the mixer of esc_trace_options, high 32 bits; 0xFFFFFFFE and 0xFFFFFFFF are taken by the
 *             ambient set and the Fresnel draw, and no light has this index)
 *       l   = table[set][k]
 *       off = U*(l.x*aperture) + V*(l.y*aperture)
 *       o'  = origin + off
 *       d'  = normalize(p*focus_dist - off)
 *
 * camera.h:16-29 puts the image plane at distance 1, so p has axial component 1 and origin + p*focus_dist
 * lies on the focus plane; the line of (o', d') passes it whatever l is.  `set` does not depend on k: the spp
 * samples of a pixel walk one set and so stay stratified over the lens.  A degenerate camera makes NaN rays,
 * as written.  With aperture == 0 nothing new is computed and the table is not read.  A lens ray is an
 * ordinary ray to the sweeps: it passes the precondition gate or runs the reference loop, as any
 * caller-supplied ray does. */
typedef struct esc_lens_options { /* 24 bytes */
  float aperture;      /* the lens radius in scene units: finite, >= 0 */
  float focus_dist;    /* distance along the view axis of the plane that stays sharp: finite, > 0 */
  uint64_t seed;       /* picks each pixel's set of the table */
  int32_t reserved[2]; /* must be 0 */
} esc_lens_options;
/* host_table: sets*samples*2 floats in HOST memory, copied to the device.  The table belongs to the context
 * and survives scene uploads; a new one replaces it; sets == 0 with host_table == NULL removes it (samples is
 * then ignored).  Synchronises the context's stream before and after.  sets or samples outside 1..64, or
 * exactly one of sets == 0 / host_table == NULL, is ESC_ERR_INVALID. */
int esc_set_lens_table(esc_context *ctx, int32_t sets, int32_t samples, const float *host_table);
/* *sets, *samples = the shape of the context's lens table, 0 and 0 when none is set */
int esc_get_lens_table_shape(esc_context *ctx, int32_t *sets, int32_t *samples);
/* A table of uniformly distributed lens points, on the host, without a context or a device, deterministic in
 * its three arguments.  out: sets*samples*2 floats.  Random numbers: splitmix64 from
 * seed ^ (sets << 48) ^ (samples << 40) ^ 0x4C454E53, u = ((x >> 11) + 0.5) * 2^-53 in (0, 1).  Per set: when
 * samples is a square n*n, cell c = j*n + i of an n x n grid gets the point ((i + u1)/n, (j + u2)/n) of the
 * unit square, otherwise point c is ((c + u1)/samples, u2); the point (a, b) = (2x - 1, 2y - 1) goes through the
 * concentric square-to-disk map (|a| > |b|: r = a, phi = (pi/4)*(b/a); else r = b, phi = pi/2 - (pi/4)*(a/b);
 * (0, 0) stays) to (r cos phi, r sin phi); then the set's points are shuffled (Fisher-Yates, j = floor(u*(m+1))
 * for m = samples-1 .. 1), so that lens sample k is not tied to sub-pixel cell k.  All in double with the
 * host's libm, then cast to float and, if the cast left x*x + y*y above 1, scaled by 1 - 2^-24 until it is
 * not.  The result is data a caller can read, store or replace.  sets or samples outside 1..64 or a null
 * pointer is ESC_ERR_INVALID. */
int esc_lens_disk_table(int32_t sets, int32_t samples, uint64_t seed, float *out);
/* The frame's primary rays through the lens, as data: esc_camera_rays' twin with the same layout, alignment,
 * n == 0 and asynchrony rules.  Ray i = (h - row_begin)*W + w of rows [row_begin, row_end) is the ray above
 * with (dx, dy) = d_offsets[2i], d_offsets[2i+1] (NULL: 0), lens sample `sample` and q = h*W + w.  Needs a
 * table and 0 <= sample < K unless lens.aperture == 0, where the rays are esc_camera_rays', bit for bit.
 * ESC_ERR_INVALID, with nothing launched: an aperture that is negative, NaN or infinite, a focus_dist that is
 * not finite or not > 0, a non-zero reserved word, a sample beyond the table, no table while aperture > 0, a
 * NULL or misaligned pointer, and esc_camera_rays' argument errors.  No scene is needed. */
int esc_lens_rays(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t row_begin,
                  int32_t row_end, const float *d_offsets, const esc_lens_options *lens, int32_t sample,
                  float *d_origins, float *d_dirs);
/* Frame with depth of field: esc_render_traced_ex with every sample's ray sent through the lens.  Sample k of
 * spp = n*n takes the grid offset of esc_render_supersampled, lens sample k, pixel id h*W + w and seed
 * opts.seed + k, and is traced as esc_trace_rays_ex traces it; the same sum in sample order, the same
 * division by float(spp) and quantisation, the same bands with at most 256 MB of scratch, and
 * esc_last_trace_stats / esc_last_transmit_stats report it.  Needs K >= spp unless lens.aperture == 0.  With
 * aperture == 0 the frame is esc_render_traced_ex's, bit for bit (and with max_depth == 0 and no environment
 * esc_render_supersampled's).  The environment rule above applies unchanged.  ESC_ERR_INVALID, with nothing
 * launched: the lens errors of esc_lens_rays (spp in place of sample) and esc_render_traced_ex's argument
 * errors.  Out of scope: a lens in the frame kernels or in the adaptive, ambient, sky-light and G-buffer
 * frames, polygonal apertures, bokeh weights, chromatic aberration, motion blur. */
int esc_render_lens(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                    const esc_render_options *opts, const esc_trace_options *trace_opts,
                    const esc_lens_options *lens, float *d_image, uint8_t *d_u8);

/* Whole frame into HOST memory, synchronous: render + D2H.  `image` = W*H*3 floats. */
int esc_render_frame_host(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                          const esc_render_options *opts, float *image, uint8_t *rgb8);

/* Single-process multi-GPU: 8-row strips dealt round-robin over n_devices (band i renders
 * strips i, i+n, ...), every band launched before any is waited on, strips copied straight
 * into the caller's host frame.  Bands share devices when there are fewer GPUs than bands.
 * (bench.py uses one process per GPU + an RCCL gather instead.) */
int esc_render_frame_multi(const esc_scene *scene, const esc_camera *cam, int32_t W, int32_t H,
                           const esc_render_options *opts, int32_t n_devices, float *image,
                           uint8_t *rgb8, float *ms_per_device /* [n_devices] or NULL */);

/* ---- native multi-GPU with an RCCL gather ------------------------
 * What a C++ host at the reference's call site (main.cpp:619-624, rows are independent:
 * main.cpp:628-636) uses to reach all GPUs of a node from ONE process: one context per device,
 * 8-row strips dealt round-robin (the esc_render_strips partition), every device renders its
 * strips, and the ONE exchange step -- the framebuffer gather to the first device -- runs over
 * RCCL: grouped ncclSend / ncclRecv, direct peer -> root over xGMI, fp32 RGB (12 B/pixel, the
 * `trace` seam's return_image) or the PPM-quantised bytes (3 B/pixel, main.cpp:676-682).  Then
 * esc_assemble_strips lays the frame out on the first device.  RCCL is bound at run time
 * (dlopen of librccl.so; $ESC_RCCL_LIB overrides), so the library itself does not link it.
 *   use_rccl = 0 replaces the exchange by hipMemcpyPeerAsync (same layout; for hosts without RCCL).
 *   With RCCL n_devices must not exceed the device count and the ids must be distinct (one
 *   communicator rank per device).  Without it ranks may SHARE devices: device_ids may repeat, and
 *   with device_ids == NULL rank i takes device i % count -- the n-rank partition, offsets, copies
 *   and assembly then run on however many GPUs there are (how a 1-GPU box tests n = 2, 3, 8).
 *   STATE OF VERIFICATION: the n > 1 path without RCCL runs in the GPU tests (ranks sharing one
 *   device); the grouped ncclSend / ncclRecv exchange has so far only run with n = 1, where it
 *   moves nothing. */
typedef struct esc_multi esc_multi;
int esc_rccl_available(void); /* 1 / 0 (esc_last_error says why not) */
int esc_multi_create(int32_t n_devices, const int32_t *device_ids /* NULL = 0..n-1 (RCCL) / i % count */,
                     int32_t use_rccl, esc_multi **out);
void esc_multi_destroy(esc_multi *m);
int esc_multi_upload_scene(esc_multi *m, const esc_scene *scene); /* replicated on every device */
/* One frame, synchronous.  gather_u8 = 0: fp32 RGB is gathered (`image` may be set, rgb8 must be
 * NULL); 1: the quantised bytes (`rgb8` may be set, image must be NULL).  Host pointers may be
 * NULL when only the device-resident frame is wanted: *d_frame (if non-NULL) receives the
 * assembled frame's address on the first device, valid until the next call on `m`. */
int esc_multi_render(esc_multi *m, const esc_camera *cam, int32_t W, int32_t H,
                     const esc_render_options *opts, int32_t gather_u8, float *image,
                     uint8_t *rgb8, void **d_frame, float *ms_per_device /* [n] or NULL */);
/* create + upload + render + destroy in one call (the shape of esc_render_frame_multi).
 * NOTE: every call creates the contexts, uploads the scene to every device AND initialises an RCCL
 * communicator (ncclCommInitAll: tens to hundreds of milliseconds), then tears all of it down.
 * Meant for a viewer's single frame; a caller that renders in a loop keeps an esc_multi. */
int esc_render_frame_multi_rccl(const esc_scene *scene, const esc_camera *cam, int32_t W, int32_t H,
                                const esc_render_options *opts, int32_t n_devices, float *image,
                                uint8_t *rgb8, float *ms_per_device /* [n_devices] or NULL */);

/* ------------------------------------------------------------------------------------
 * PPM writer == main.cpp:658-689: "P3\nW H\n255\n", rows top-down, clamp >1, int(c*255)
 * ---------------------------------------------------------------------------------- */
int esc_write_ppm(const char *path, const float *image, int32_t W, int32_t H);
/* same text from already-quantised bytes (same (h*W+w)*3 order) */
int esc_write_ppm_u8(const char *path, const uint8_t *rgb8, int32_t W, int32_t H);
void esc_quantise(const float *image, int64_t n_values, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* ESCTP1_RT_H */
