// rt_capi.cpp -- device half of the C ABI (include/esctp1_rt.h): context, scene staging
// into HBM, row-band rendering, the `trace` drop-in.  HIP runtime API only; the kernels live
// in rt_kernels.hip.  There is deliberately no CPU rendering path in this library: without a
// gfx950 device every render entry point fails with ESC_ERR_NO_DEVICE / ESC_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/accel_build.h"
#include "../host/scene.h"
#include "../host/scene_tables.h"
#include "rt_adaptive.h"
#include "rt_ambient.h"
#include "rt_environ.h"
#include "rt_device.h"
#include "rt_devmem.h"
#include "rt_filter.h"
#include "rt_gbuffer.h"
#include "rt_lens.h"
#include "rt_query.h"
#include "rt_shade_rays.h"
#include "rt_temporal.h"
#include "rt_trace.h"
#include "rt_tile_math.h"

static_assert(sizeof(esc_bvh_node) == sizeof(esc::BvhNode) && sizeof(esc::BvhNode) == 64,
              "esc_bvh_node is the public face of esc::BvhNode");

extern "C" int esc_launch_prepare(const esc::RenderParams *p, esc::DevTriP *tri_p,
                                  esc::DevTriF *tri_f, esc::DevTriPF *tri_pf, esc::DevSphP *sph_p,
                                  esc::DevSphF *sph_f, const esc::SphGroups *sg,
                                  const esc::TriGroups *tg, hipStream_t stream);
extern "C" int esc_launch_face_normals(const esc::DevTri *tri, esc::DevTriFace *out, int n, hipStream_t stream);
extern "C" int esc_launch_prepare_bvh(const esc::DevTri *tri, esc::DevTriP *tri_p, int n_tri,
                                      const esc::DevSph *sph, esc::DevSphP *sph_p, int n_sph,
                                      float ox, float oy, float oz, hipStream_t stream);
extern "C" int esc_launch_tile_lists(const esc::RenderParams *p, hipStream_t stream);
extern "C" int esc_launch_light_lists(const esc::RenderParams *p, hipStream_t stream);
extern "C" int esc_launch_light_pack(const esc::RenderParams *p, int fill, hipStream_t stream);
extern "C" int esc_launch_bin_primary(const esc::RenderParams *p, const esc::PrimBoxDev *tri_boxes,
                                      const esc::PrimBoxDev *sph_boxes, hipStream_t stream);
extern "C" int esc_launch_bin_light(const esc::LightBins *g, const float *light_points,
                                    const esc::PrimBoxDev *tri_boxes, int n_tri,
                                    const esc::PrimBoxDev *sph_boxes, int n_sph,
                                    hipStream_t stream);
extern "C" int esc_launch_ray_tables(const esc::RenderParams *p, esc::RayEntry *col, esc::RayEntry *row,
                                     hipStream_t stream);
extern "C" int esc_launch_check_inv_det(uint32_t first, uint64_t n, unsigned long long *out, hipStream_t stream);
extern "C" int esc_launch_render(const esc::RenderParams *p, const esc::RayTables *rays, int stage, int px,
                                 hipStream_t stream, hipEvent_t between, int two_kernels, int *which);
extern "C" int esc_launch_shade_queue(const esc::RenderParams *p, int li, int last, const int *segs,
                                      int n_segs, uint32_t *ctl, int n_wg, hipStream_t stream);
extern "C" int esc_launch_primary_only(const esc::RenderParams *p, int px, hipStream_t stream);
extern "C" int esc_launch_query(const esc::QueryParams *p, int occlusion, hipStream_t stream);
extern "C" int esc_launch_shade_rays(const esc::ShadeParams *p, hipStream_t stream);
extern "C" int esc_launch_camera_rays(const esc::CameraRayParams *p, hipStream_t stream);
extern "C" int esc_launch_ss_accumulate(float *acc, const float *rgb, int64_t n, int first, hipStream_t stream);
extern "C" int esc_launch_ss_finish(float *img, uint8_t *u8, int64_t n, float spp, hipStream_t stream);
extern "C" int esc_launch_trace_level(const esc::TraceParams *p, hipStream_t stream);
extern "C" int esc_launch_adaptive_mask(const esc::AdaptiveMaskParams *p, hipStream_t stream);
extern "C" int esc_launch_adaptive_list(const esc::AdaptiveListParams *p, hipStream_t stream);
extern "C" int esc_launch_adaptive_refine(const esc::AdaptiveRefineParams *p, hipStream_t stream);
extern "C" int esc_launch_ambient(const esc::AmbientParams *p, int camera, int sky, hipStream_t stream);
extern "C" int esc_launch_add_light(const esc::AddLightParams *p, hipStream_t stream);
extern "C" int esc_launch_environment_rays(const esc::EnvRaysParams *p, hipStream_t stream);
extern "C" int esc_launch_lens_rays(const esc::LensRayParams *p, hipStream_t stream);
extern "C" int esc_launch_modulate(const esc::ModulateParams *p, hipStream_t stream);
extern "C" int esc_launch_gbuffer(const esc::GBufferParams *p, int camera, hipStream_t stream);
extern "C" int esc_launch_filter_pack(const esc::FilterPackParams *p, hipStream_t stream);
extern "C" int esc_launch_filter_atrous(const esc::FilterParams *p, int channels, int64_t tiles, hipStream_t stream);
extern "C" int esc_launch_temporal(const esc::TemporalParams *p, int channels, int taps, int64_t tiles,
                                   hipStream_t stream);
extern "C" int esc_launch_assemble(const void *gathered, void *frame, size_t rank_pitch_bytes,
                                   int n_ranks, int H, int strip_rows, size_t row_bytes,
                                   hipStream_t stream);

using esc::set_error;
using esc::stage_flat;
using esc::stage_scene;
using esc::Staged;

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                        \
      return ESC_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

struct esc_context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // staged scene (HBM)
  esc::DevTri *d_tri = nullptr;
  esc::DevTriP *d_tri_p = nullptr;
  esc::DevTriN *d_tri_n = nullptr;
  esc::DevTriFace *d_tri_face = nullptr;
  esc::DevSph *d_sph = nullptr;
  esc::DevSphP *d_sph_p = nullptr;
  esc::DevSphPair *d_sph2 = nullptr;
  esc::DevSphF *d_sph_f = nullptr;      // filter forms (rt_brute.h "FILTERS")
  esc::DevSphPairF *d_sph2_f = nullptr;
  esc::DevSphPair *d_sph2_ord = nullptr;    // last light's sweep order (rt_device.h sph2_ord)
  esc::DevSphPairF *d_sph2_f_ord = nullptr;
  esc::SphGroups sg{};                  // sphere groups
  esc::TriGroups tg{};                  // triangle groups
  esc::DevTriF *d_tri_f = nullptr;
  esc::DevTriPairF *d_tri2_f = nullptr;
  esc::DevTriPF *d_tri_pf = nullptr;       // pre-filter forms (rt_brute.h "Triangle pre-filter")
  esc::DevTriPairPF *d_tri2_pf = nullptr;
  float shadow_center[3] = {0, 0, 0};
  float shadow_rho_max = 0.f;
  float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0}; // grown scene box (light lists)
  int32_t *d_sph_mat = nullptr;
  esc::DevMat *d_mat = nullptr;
  esc::DevLight *d_lights = nullptr;
  float *d_light_points = nullptr;
  unsigned long long *d_counters = nullptr;
  int n_tri = 0, n_sph = 0, n_lights = 0, n_geom = 0;
  int min_light_faces = 0; // smallest face count among the lights (bounds ESC_FACE_FIXED)
  bool have_scene = false;
  // bumped whenever per-camera / per-scene device state is rebuilt (prepare kernels, tile and light
  // lists, the tree, scratch buffers): a recorded frame (esc_frame) replays launches that read that
  // state and is only valid for the epoch it was recorded in
  uint64_t epoch = 0;
  bool capturing = false; // inside esc_frame_record's stream capture: nothing may rebuild
  // every device buffer below (and inside sg, tg, sl, tl, ll, lt, lbins) is allocated through one of
  // these two and freed with it (rt_devmem.h).  `frame`: what a kernel launched by esc_render_strips
  // reads or writes -- the staged scene and its tables, d_hits, the lists, the tree, the bins, d_sq,
  // d_sq_ctl, d_counters; freeing any of it ends every recorded frame.  `call`: everything else
  esc::DevMem frame{this, &epoch, &capturing};
  esc::DevMem call{this};
  bool prepared = false;
  float prepared_origin[3] = {0, 0, 0};
  // k_frame's ray tables (rt_device.h RayTables): W and H entries, valid for ray_key; grow-only
  esc::RayEntry *d_ray_col = nullptr, *d_ray_row = nullptr;
  size_t ray_col_cap = 0, ray_row_cap = 0;
  struct RayKey {
    float cam[9]; // lower_left_corner, horizontal, vertical (the origin is subtracted per pixel)
    int32_t W, H;
  } ray_key{};
  bool rays_valid = false;
  int32_t *d_hits = nullptr; // k_primary -> k_shade hand-over: 3 planes (idx, t, v) of hits_cap / 3 dwords
  size_t hits_cap = 0;
  // tile lists of the primary pass (rt_device.h TileLists), valid for list_key
  esc::TileLists sl{}, tl{};
  size_t list_tiles_cap = 0;
  struct ListKey {
    float cam[12];
    int32_t W, H, h0, n_local_rows, strip_rows, strip_step, n_sg, n_tg;
    int32_t n_mask_tri; // > 0: tl.cnt holds the triangle masks of that many directly swept triangles
  } list_key{};
  bool lists_valid = false;
  bool tri_masks_last = false; // the last frame asked for the masks (and list_key describes them)
  bool list_ids_stale = false; // a new scene: ids of the old one may be out of range
  // light lists of the shadow pass (rt_device.h LightLists), valid for (scene, ll_face_mode, ll_fixed_face)
  esc::LightLists ll{}, lt{}; // sphere / triangle pair records
  int ll_alloc_lights = 0;
  size_t ll_pk_steps_cap = 0; // steps ll.pk_rec / ll.pk_pos hold (the spare step not counted)
  int32_t ll_pk_steps = -1;   // steps the packed cells of the valid lists use; < 0: not built for them
  int ll_face_mode = -1, ll_fixed_face = -1;
  bool ll_valid = false;
  // no cell or face of the valid sphere lists is one the sweep refuses (light_list_refused, counted by
  // k_pack_light_cells<false> and read back with the step total)
  bool ll_complete = false;
  // "every shadow origin of this camera lies in the grown box" (esc::shadow_origins_inside), per camera
  // origin and scene; sure_epoch: the scene it was asked of
  float sure_origin[3] = {0, 0, 0};
  bool sure_inside = false, sure_known = false;
  int last_frame_kernel = 0;     // ESC_FRAME_KERNEL_* bits of the last frame (esc_last_frame_kernel)
  std::vector<esc::DevLight> h_lights;
  // ESC_STAGE_BVH: host copy of the tables the builder reads, the tree in HBM
  std::vector<esc::DevTri> h_tri;
  std::vector<esc::DevSph> h_sph;
  std::vector<float> h_light_points;
  esc::BvhNode *d_bvh_tri_nodes = nullptr, *d_bvh_sph_nodes = nullptr;
  esc::TriBlock *d_bvh_tri_blocks = nullptr;
  esc::SphBlock *d_bvh_sph_blocks = nullptr;
  int32_t *d_bvh_tri_order = nullptr, *d_bvh_sph_order = nullptr;
  esc::TriBlockP *d_bvh_tri_blocks_p = nullptr; // hoisted for accel_prepared_origin
  esc::SphBlockP *d_bvh_sph_blocks_p = nullptr;
  bool accel_prepared = false;
  float accel_prepared_origin[3] = {0, 0, 0};
  // screen-space bins of the primary pass (rt_device.h BinGrid)
  esc::PrimBoxDev *d_tri_boxes = nullptr, *d_sph_boxes = nullptr;
  int32_t *d_bin_hdr = nullptr, *d_bin_tri_ids = nullptr, *d_bin_sph_ids = nullptr;
  int bin_tiles_x = 0, bin_groups_y = 0;
  // light-space bins of the shadow pass (rt_device.h LightBins), built with the tree
  esc::LightBins lbins{};
  bool accel_valid = false;
  esc::OriginBounds accel_ob{};
  esc_accel_info accel_info{};
  // queue form of the shadow pass (rt_device.h ShadeQueue): grow-only scratch
  char *d_sq = nullptr;
  size_t sq_bytes = 0;
  uint32_t *d_sq_ctl = nullptr;
  size_t sq_ctl_words = 0;
  int n_cu = 0;
  // ESC_RENDER_TIME_KERNELS: events around / between the two frame kernels of the last frame
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ev_valid = false;
  // scratch framebuffers for esc_render_frame_host
  float *d_img = nullptr;
  uint8_t *d_u8 = nullptr;
  size_t img_cap = 0, u8_cap = 0;
  // esc_query_stats of the last ray query (rt_query.hip), allocated by the first query
  unsigned long long *d_qstats = nullptr;
  // esc_shade_stats of the last esc_shade_rays call (rt_shade_rays.hip), allocated by the first one
  unsigned long long *d_sstats = nullptr;
  // esc_render_supersampled: one band's rays and colours (grow-only, at most kSsScratchBytes)
  float *d_ss = nullptr;
  size_t ss_floats = 0;
  // esc_trace_rays / esc_render_traced (rt_trace.hip): esc_trace_stats + the queue counters, and one
  // batch's queues (plus, for a frame, its rays and colours); grow-only, at most kSsScratchBytes
  unsigned long long *d_tstats = nullptr;
  float *d_tr = nullptr;
  size_t tr_floats = 0;
  // transmission side table (tf[3], ni per material, indexed like d_mat) of esc_trace_rays_ex, and
  // whether any of its entries is transmissive: only then do the TRANSMIT kernels run
  float *d_transmit = nullptr;
  bool any_transmissive = false;
  // esc_render_adaptive (rt_adaptive.hip): esc_adaptive_stats' device counters + the list's counter,
  // and the scratch (grow-only): 4 bytes per list slot of a band, then 1 byte per pixel for the mask
  // when the caller passes none.  ad_pixels / ad_spp: the last call's frame and spp, for the stats
  unsigned long long *d_astats = nullptr;
  uint8_t *d_ad = nullptr;
  size_t ad_bytes = 0;
  uint64_t ad_pixels = 0;
  int32_t ad_spp = 0;
  // ambient occlusion (rt_ambient.hip): the sample table of esc_set_ambient_table (am_sets x am_samples x 3
  // floats; the context's, not the scene's: an upload leaves it alone), esc_ambient_stats' device
  // counters and the last call's K
  float *d_am_table = nullptr;
  int32_t am_sets = 0, am_samples = 0;
  unsigned long long *d_amstats = nullptr;
  int32_t am_k = 0;
  // the environment cube of esc_set_environment (rt_environ.h): 6 * env_res^2 records of 16 bytes; the
  // context's, not the scene's.  nullptr: traced rays that miss stay black
  esc::EnvTexel *d_env = nullptr;
  int32_t env_res = 0;
  // the lens table of esc_set_lens_table (rt_lens.h): lens_sets x lens_samples x 2 floats, points of the unit
  // disk; the context's, not the scene's.  nullptr: only aperture 0 renders
  float *d_lens = nullptr;
  int32_t lens_sets = 0, lens_samples = 0;
  // the G-buffer (rt_gbuffer.hip): esc_gbuffer_stats' device counters, allocated by the first call
  unsigned long long *d_gbstats = nullptr;
  // esc_filter_guided (rt_filter.hip): esc_filter_stats' device counters and the last call's W*H, and the
  // scratch (grow-only): one 32-byte guide record per pixel, and one image for the iterations to alternate with
  unsigned long long *d_flstats = nullptr;
  uint64_t fl_pixels = 0;
  esc::FilterGuide *d_fl_guide = nullptr;
  size_t fl_guide_cap = 0;
  float *d_fl_img = nullptr;
  size_t fl_img_cap = 0;
  // esc_temporal_accumulate (rt_temporal.hip): esc_temporal_stats' device counters (kTemporalStatSets replicas
  // of 8 words, summed on read) and the last call's W*H
  unsigned long long *d_tpstats = nullptr;
  uint64_t tp_pixels = 0;
};

// ---- rt_devmem.h's backend: the only hipMalloc / hipFree of this file
static std::atomic<int64_t> g_live_buffers{0}, g_live_bytes{0};

void *esc::devmem_allocate(size_t bytes) {
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return nullptr;
  }
  g_live_buffers++;
  g_live_bytes += (int64_t)bytes;
  return p;
}

void esc::devmem_free(void *p, size_t bytes) {
  (void)hipFree(p);
  g_live_buffers--;
  g_live_bytes -= (int64_t)bytes;
}

bool esc::devmem_wait(void *owner) {
  const hipError_t e = hipStreamSynchronize(static_cast<const esc_context *>(owner)->stream);
  if (e != hipSuccess) set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  return e == hipSuccess;
}

namespace {

// P: T, or const T for the tables the kernels only read
template <typename P, typename T>
int upload_vec(esc::DevMem &mem, P *&dptr, const std::vector<T> &h, hipStream_t st) {
  const int rc = mem.alloc(dptr, h.size());
  if (rc || h.empty()) return rc;
  HIP_TRY(hipMemcpyAsync(const_cast<T *>(dptr), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return ESC_OK;
}

int commit(esc_context *ctx, const Staged &s) {
  HIP_TRY(hipSetDevice(ctx->device));
  esc::SceneTables t;
  esc::build_scene_tables(s, t);
  std::memcpy(ctx->scene_lo, t.scene_lo, sizeof(t.scene_lo));
  std::memcpy(ctx->scene_hi, t.scene_hi, sizeof(t.scene_hi));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // nothing in flight may still read old tables
  int rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.sorted, t.tg_sorted, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.orig, t.tg_orig, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.grp, t.tg_grp, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.sorted2_pf, t.tg_sorted2_pf, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.sorted2_f, t.tg_sorted2_f, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->tg.grp2_pf, t.tg_grp2_pf, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->tg.sorted_p, t.tg_sorted.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->tg.sorted_f, t.tg_sorted.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->tg.sorted_pf, t.tg_sorted.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->tg.grp_pf, t.tg_grp.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->tg.esc, 3 * t.tg_grp.size()))) return rc; // three chains (rt_device.h)
  ctx->tg.n_grp = t.tg_n_grp;
  ctx->tg.n_sup = t.tg_n_sup;
  ctx->tg.n_hyp = t.tg_n_hyp;
  if ((rc = upload_vec(ctx->frame, ctx->sg.sorted2, t.sg_sorted2, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->sg.sorted2_f, t.sg_sorted2_f, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->sg.grp2_f, t.sg_grp2_f, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->sg.sorted, t.sg_sorted, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->sg.grp, t.sg_grp, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->sg.orig, t.sg_orig, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->sg.sorted_p, t.sg_sorted.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->sg.sorted_f, t.sg_sorted.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->sg.grp_f, t.sg_grp.size()))) return rc;
  ctx->sg.n_grp = t.sg_n_grp;
  ctx->sg.n_sup = t.sg_n_sup;
  ctx->sg.n_hyp = t.sg_n_hyp;
  if ((rc = upload_vec(ctx->frame, ctx->d_sph2_ord, t.sph2_ord, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_sph2_f_ord, t.sph2_f_ord, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_sph2_f, t.sph2_f, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_sph_f, s.sph.size()))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_tri2_f, t.tri2_f, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_tri_f, s.tri.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_tri_pf, s.tri.size()))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_tri2_pf, t.tri2_pf, ctx->stream))) return rc;
  std::memcpy(ctx->shadow_center, t.g, sizeof(t.g));
  ctx->shadow_rho_max = t.rho_max;
  if ((rc = upload_vec(ctx->frame, ctx->d_tri, s.tri, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_tri_n, s.tri_n, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_tri_face, s.tri.size()))) return rc;
  if (!s.tri.empty()) {
    const int e = esc_launch_face_normals(ctx->d_tri, ctx->d_tri_face, (int)s.tri.size(), ctx->stream);
    if (e) {
      set_error(std::string("k_prepare_face_normals launch: ") + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  if ((rc = upload_vec(ctx->frame, ctx->d_sph, s.sph, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_sph2, t.sph2, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_sph_mat, s.sph_mat, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_mat, s.mat, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->call, ctx->d_transmit, s.transmit, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_lights, s.lights, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_light_points, s.light_points, ctx->stream))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_tri_p, s.tri.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_sph_p, s.sph.size()))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // host vectors die with the caller's frame
  ctx->n_tri = (int)s.tri.size();
  ctx->n_sph = (int)s.sph.size();
  ctx->n_lights = (int)s.lights.size();
  ctx->n_geom = s.n_geom;
  ctx->any_transmissive = t.any_transmissive;
  ctx->min_light_faces = t.min_light_faces;
  ctx->have_scene = true;
  ctx->epoch++;
  ctx->prepared = false;
  ctx->lists_valid = false;
  ctx->list_ids_stale = true;
  ctx->ll_valid = false;
  ctx->ll_complete = false;
  ctx->sure_known = false;
  ctx->h_lights = s.lights;
  ctx->h_tri = s.tri;
  ctx->h_sph = s.sph;
  ctx->h_light_points = s.light_points;
  ctx->accel_valid = false;
  return ESC_OK;
}

// ---- acceleration structure: host build (accel_build.cpp) + leaf blocks in tree order
struct AccelHost {
  esc::BuiltBvh tri, sph;
  std::vector<esc::TriBlock> tri_blocks;
  std::vector<esc::SphBlock> sph_blocks;
  std::vector<esc::PrimBox> tri_boxes, sph_boxes;
  esc::OriginBounds ob;
};

void build_accel_host(const std::vector<esc::DevTri> &tri, const std::vector<esc::DevSph> &sph,
                      const std::vector<float> &light_points, const float origin[3],
                      AccelHost &a) {
  a.ob = esc::origin_bounds(tri, sph, light_points, origin);
  esc::triangle_boxes(tri, a.ob, a.tri_boxes);
  esc::sphere_boxes(sph, a.ob, a.sph_boxes);
  esc::build_bvh(a.tri_boxes, esc::kTriBlock, 0u, esc::kBvhMaxDepth, a.tri);
  esc::build_bvh(a.sph_boxes, esc::kSphBlock, (uint32_t)tri.size(), esc::kBvhMaxDepth, a.sph);
  a.tri_blocks.resize((size_t)a.tri.n_blocks);
  for (size_t i = 0; i < a.tri.order.size(); i++) {
    esc::DevTri &dst = a.tri_blocks[i / esc::kTriBlock].t[i % esc::kTriBlock];
    if (a.tri.order[i] >= 0)
      dst = tri[(size_t)a.tri.order[i]];
    else
      std::memset(&dst, 0, sizeof(dst)); // e1 = e2 = 0: det = 0, rejected at ray_triangle.h:23
  }
  a.sph_blocks.resize((size_t)a.sph.n_blocks);
  for (size_t i = 0; i < a.sph.order.size(); i++) {
    esc::DevSph &dst = a.sph_blocks[i / esc::kSphBlock].s[i % esc::kSphBlock];
    if (a.sph.order[i] >= 0) {
      dst = sph[(size_t)a.sph.order[i]];
    } else { // disc = b*b - (|oc|^2 + inf) = -inf: never a hit
      dst.cx = dst.cy = dst.cz = 0.f;
      dst.r2 = -__builtin_huge_valf();
    }
  }
}

void fill_info(const AccelHost &a, esc_accel_info &info) {
  info.tri_nodes = (int32_t)a.tri.nodes.size();
  info.tri_blocks = a.tri.n_blocks;
  info.tri_depth = a.tri.depth;
  info.tri_root = a.tri.root;
  info.sph_nodes = (int32_t)a.sph.nodes.size();
  info.sph_blocks = a.sph.n_blocks;
  info.sph_depth = a.sph.depth;
  info.sph_root = a.sph.root;
}

int build_accel_device(esc_context *ctx, const float origin[3]) {
  const auto t0 = std::chrono::steady_clock::now();
  AccelHost a;
  build_accel_host(ctx->h_tri, ctx->h_sph, ctx->h_light_points, origin, a);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // no frame in flight may still walk the old tree
  int rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_tri_nodes, a.tri.nodes, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_tri_blocks, a.tri_blocks, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_tri_order, a.tri.order, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_sph_nodes, a.sph.nodes, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_sph_blocks, a.sph_blocks, ctx->stream))) return rc;
  if ((rc = upload_vec(ctx->frame, ctx->d_bvh_sph_order, a.sph.order, ctx->stream))) return rc;
  static_assert(sizeof(esc::PrimBox) == sizeof(esc::PrimBoxDev), "same six floats");
  {
    std::vector<esc::PrimBoxDev> tb(a.tri_boxes.size()), sb(a.sph_boxes.size());
    if (!tb.empty()) std::memcpy(tb.data(), a.tri_boxes.data(), tb.size() * sizeof(esc::PrimBoxDev));
    if (!sb.empty()) std::memcpy(sb.data(), a.sph_boxes.data(), sb.size() * sizeof(esc::PrimBoxDev));
    if ((rc = upload_vec(ctx->frame, ctx->d_tri_boxes, tb, ctx->stream))) return rc;
    if ((rc = upload_vec(ctx->frame, ctx->d_sph_boxes, sb, ctx->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // tb / sb die here
  }
  ctx->bin_tiles_x = ctx->bin_groups_y = 0; // bins hold ids of the old scene: start over
  {
    // cube maps around the light sample points (they belong to the scene, not to the camera)
    const int n_pts = (int)(ctx->h_light_points.size() / 4);
    const size_t n_prims = ctx->h_tri.size() + ctx->h_sph.size();
    esc::LightBins &g = ctx->lbins;
    g.n_points = 0;
    if (n_pts >= 1 && n_pts <= esc::kLightGridsMax && n_prims > 0) {
      // cells per cube-face edge, measured (frame ms at R = 64 / 128 / 256): c3 0.217 / 0.213 /
      // 0.215, c4 0.265 / 0.260 / 0.257, c5 1.21 / 1.13 / 1.00 -- finer pays once a cell would
      // otherwise overflow; 26 MB per light point at 128, 104 MB at 256
      g.R = n_prims <= 32768 ? 128 : 256;
      const size_t n_cells = (size_t)n_pts * 6 * g.R * g.R;
      if ((rc = ctx->frame.alloc(g.face_hdr, (size_t)n_pts * 6 * esc::kBinHdrInts))) return rc;
      if ((rc = ctx->frame.alloc(g.counts, 2 * n_cells))) return rc;
      if ((rc = ctx->frame.alloc(g.tri_ids, n_cells * esc::kBinCap))) return rc;
      if ((rc = ctx->frame.alloc(g.sph_ids, n_cells * esc::kBinCap))) return rc;
      HIP_TRY(hipMemsetAsync(g.face_hdr, 0, (size_t)n_pts * 6 * esc::kBinHdrInts * 4, ctx->stream));
      HIP_TRY(hipMemsetAsync(g.counts, 0, 2 * n_cells * 4, ctx->stream));
      HIP_TRY(hipMemsetAsync(g.tri_ids, 0, n_cells * esc::kBinCap * 4, ctx->stream));
      HIP_TRY(hipMemsetAsync(g.sph_ids, 0, n_cells * esc::kBinCap * 4, ctx->stream));
      g.n_points = n_pts;
      int e = esc_launch_bin_light(&g, ctx->d_light_points, ctx->d_tri_boxes, (int)ctx->h_tri.size(),
                                   ctx->d_sph_boxes, (int)ctx->h_sph.size(), ctx->stream);
      if (e) {
        set_error(std::string("k_bin_light launch: ") + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
    }
  }
  if ((rc = ctx->frame.alloc(ctx->d_bvh_tri_blocks_p, a.tri_blocks.size()))) return rc;
  if ((rc = ctx->frame.alloc(ctx->d_bvh_sph_blocks_p, a.sph_blocks.size()))) return rc;
  ctx->accel_prepared = false;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int builds = ctx->accel_info.builds;
  std::memset(&ctx->accel_info, 0, sizeof(ctx->accel_info));
  fill_info(a, ctx->accel_info);
  ctx->accel_info.builds = builds + 1;
  ctx->accel_info.build_ms =
      std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ctx->accel_ob = a.ob;
  ctx->accel_valid = true;
  ctx->epoch++;
  return ESC_OK;
}

} // namespace

extern "C" {

int esc_context_create(int32_t device, esc_context **out) {
  if (!out) {
    set_error("esc_context_create: out is null");
    return ESC_ERR_INVALID;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error(std::string("no HIP device available (") +
              (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
              "); this renderer has no CPU fallback");
    return ESC_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    set_error("esc_context_create: device index out of range");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  esc_context *ctx = new (std::nothrow) esc_context();
  if (!ctx) return ESC_ERR_NOMEM;
  ctx->device = device;
  hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (se != hipSuccess) {
    set_error(std::string("hipStreamCreate: ") + hipGetErrorString(se));
    delete ctx;
    return ESC_ERR_HIP;
  }
  ctx->own_stream = true;
  int rc = ctx->frame.alloc(ctx->d_counters, (size_t)esc::kCounterSets * 8);
  if (rc == ESC_OK) {
    const hipError_t ce = hipMemset(ctx->d_counters, 0, esc::kCounterSets * 8 * sizeof(unsigned long long));
    if (ce != hipSuccess) {
      set_error(std::string("hipMemset(counters): ") + hipGetErrorString(ce));
      rc = ESC_ERR_HIP;
    }
  }
  if (rc != ESC_OK) {
    esc_context_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return ESC_OK;
}

void esc_context_destroy(esc_context *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (hipEvent_t ev : ctx->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx; // its two owners free every device buffer
}

int esc_context_set_stream(esc_context *ctx, void *hip_stream) {
  if (!ctx) {
    set_error("esc_context_set_stream: ctx is null");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  ctx->stream = (hipStream_t)hip_stream;
  ctx->own_stream = false;
  return ESC_OK;
}

void *esc_context_stream(esc_context *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int esc_context_synchronize(esc_context *ctx) {
  if (!ctx) {
    set_error("esc_context_synchronize: ctx is null");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ESC_OK;
}

int esc_upload_scene(esc_context *ctx, const esc_scene *scene) {
  if (!ctx || !scene) {
    set_error("esc_upload_scene: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  int rc = stage_scene(*scene, s);
  if (rc) return rc;
  return commit(ctx, s);
}

int esc_build_accel(esc_context *ctx, const float origin[3]) {
  if (!ctx || !origin) {
    set_error("esc_build_accel: bad argument");
    return ESC_ERR_INVALID;
  }
  if (!ctx->have_scene) {
    set_error("esc_build_accel: no scene uploaded");
    return ESC_ERR_INVALID;
  }
  return build_accel_device(ctx, origin);
}

int esc_get_accel_info(esc_context *ctx, esc_accel_info *out) {
  if (!ctx || !out) {
    set_error("esc_get_accel_info: bad argument");
    return ESC_ERR_INVALID;
  }
  *out = ctx->accel_info;
  return ESC_OK;
}

int esc_scene_build_accel(const esc_scene *scene, const float origin[3], int32_t which,
                          esc_accel_info *info, esc_bvh_node *nodes, int64_t nodes_cap,
                          int32_t *order, int64_t order_cap, float *prim_boxes,
                          int64_t prim_boxes_cap) {
  if (!scene || !origin || (which != 0 && which != 1)) {
    set_error("esc_scene_build_accel: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  int rc = stage_scene(*scene, s);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  AccelHost a;
  build_accel_host(s.tri, s.sph, s.light_points, origin, a);
  const esc::BuiltBvh &b = which ? a.sph : a.tri;
  const std::vector<esc::PrimBox> &boxes = which ? a.sph_boxes : a.tri_boxes;
  if ((nodes && nodes_cap < (int64_t)b.nodes.size()) ||
      (order && order_cap < (int64_t)b.order.size()) ||
      (prim_boxes && prim_boxes_cap < (int64_t)boxes.size() * 6)) {
    set_error("esc_scene_build_accel: output buffer too small");
    return ESC_ERR_INVALID;
  }
  if (nodes && !b.nodes.empty()) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(esc::BvhNode));
  if (order && !b.order.empty()) std::memcpy(order, b.order.data(), b.order.size() * sizeof(int32_t));
  if (prim_boxes && !boxes.empty()) std::memcpy(prim_boxes, boxes.data(), boxes.size() * sizeof(esc::PrimBox));
  if (info) {
    std::memset(info, 0, sizeof(*info));
    fill_info(a, *info);
    info->builds = 1;
    info->build_ms =
        std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return ESC_OK;
}

int64_t esc_scene_table(const esc_scene *scene, int32_t which, void *out, int64_t capacity) {
  if (!scene || which < 0 || which >= ESC_TABLE_COUNT || capacity < 0) {
    set_error("esc_scene_table: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  int rc = stage_scene(*scene, s);
  if (rc) return rc;
  esc::SceneTables t;
  esc::build_scene_tables(s, t);
  esc_scene_table_header hdr;
  std::memset(&hdr, 0, sizeof(hdr));
  std::memcpy(hdr.g, t.g, sizeof(hdr.g));
  hdr.rho_max = t.rho_max;
  std::memcpy(hdr.scene_lo, t.scene_lo, sizeof(hdr.scene_lo));
  std::memcpy(hdr.scene_hi, t.scene_hi, sizeof(hdr.scene_hi));
  const int32_t counts[8] = {t.sg_n_grp, t.sg_n_sup, t.sg_n_hyp, t.tg_n_grp, t.tg_n_sup, t.tg_n_hyp,
                             t.any_transmissive ? 1 : 0, t.min_light_faces};
  std::memcpy(&hdr.sg_n_grp, counts, sizeof(counts));
  auto bytes = [](const auto &v) { return std::make_pair((const void *)v.data(), v.size() * sizeof(v[0])); };
  const std::pair<const void *, size_t> tables[ESC_TABLE_COUNT] = {
      bytes(s.tri), bytes(s.tri_n), bytes(s.sph), bytes(s.sph_mat), bytes(s.mat), bytes(s.transmit),
      bytes(s.lights), bytes(s.light_points), bytes(t.sph2), bytes(t.sph2_f), bytes(t.sph2_ord),
      bytes(t.sph2_f_ord), bytes(t.tri2_f), bytes(t.tri2_pf), bytes(t.sg_sorted), bytes(t.sg_grp),
      bytes(t.sg_orig), bytes(t.sg_sorted2), bytes(t.sg_sorted2_f), bytes(t.sg_grp2_f),
      bytes(t.tg_sorted), bytes(t.tg_grp), bytes(t.tg_orig), bytes(t.tg_sorted2_f),
      bytes(t.tg_sorted2_pf), bytes(t.tg_grp2_pf), {&hdr, sizeof(hdr)}};
  const auto &tab = tables[which];
  if (out && tab.second && capacity >= (int64_t)tab.second) std::memcpy(out, tab.first, tab.second);
  return (int64_t)tab.second;
}

int esc_check_flat(int32_t num_triangles, const ispc_triangle *triangles, int32_t num_lights,
                   const ispc_light *lights, int32_t num_light_triangles,
                   const ispc_triangle *light_triangles) {
  if (num_triangles < 0 || num_lights < 0 || num_light_triangles < 0 ||
      (num_triangles && !triangles) || (num_lights && !lights) ||
      (num_light_triangles && !light_triangles)) {
    set_error("esc_check_flat: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  return stage_flat(num_triangles, triangles, num_lights, lights, num_light_triangles,
                    light_triangles, s);
}

int esc_upload_flat(esc_context *ctx, int32_t num_triangles, const ispc_triangle *triangles,
                    int32_t num_lights, const ispc_light *lights, int32_t num_light_triangles,
                    const ispc_triangle *light_triangles) {
  if (!ctx || num_triangles < 0 || num_lights < 0 || num_light_triangles < 0 ||
      (num_triangles && !triangles) || (num_lights && !lights) ||
      (num_light_triangles && !light_triangles)) {
    set_error("esc_upload_flat: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  int rc = stage_flat(num_triangles, triangles, num_lights, lights, num_light_triangles,
                      light_triangles, s);
  if (rc) return rc;
  return commit(ctx, s);
}

} // extern "C"

namespace {

constexpr int kQueueMinPrims = 2048; // below this the fused k_shade is used
// ... and below this many pixels in the band: the queue form's ~10 launches cost ~35 us each, which a
// small band (a rank's share of an 8-GPU frame) does not earn back.  Measured, rank 0's share of a
// c4 frame on one GPU, two frames in flight (tools/rank_share_time.py), queue / fused: N=1 8.27 /
// 8.98 ms, N=2 3.98 / 4.37, N=4 2.16 / 2.21, N=8 1.30 / 1.18
constexpr int64_t kQueueMinPixels = 1500000;
constexpr int kQueueMaxSegs = 48;
constexpr int kQueueFewTris = 64;   // this few triangles ride along with the first sphere segment

// segments of occlusion()'s primitive list: triangles first (index order), then sphere pair
// records.  Short segments at the start, where rays retire fastest per primitive; the length is
// raised when the list would need more than kQueueMaxSegs launches.  $ESC_QUEUE_SEG=<records>
// sets the length of the sphere segments (tuning).
void queue_segments(int n_tri, int n_sph, std::vector<int> &segs) {
  segs.clear();
  auto cut = [&](bool tris, int n, int first_len, int steady_len, int align) {
    int len = first_len, k = 0, made = 0;
    const int budget = kQueueMaxSegs / 2;
    while (k < n) {
      int left_segs = budget - made;
      int want = (made < 2) ? len : steady_len;
      if (left_segs <= 1) want = n - k;
      else want = std::max(want, (n - k + left_segs - 1) / left_segs);
      want = (want + align - 1) / align * align;
      const int c = std::min(want, n - k);
      const int seg[4] = {tris ? k : 0, tris ? c : 0, tris ? 0 : k, tris ? 0 : c};
      segs.insert(segs.end(), seg, seg + 4);
      k += c;
      made++;
    }
  };
  // $ESC_QUEUE_SEG=<records> or <first>:<steady> (tuning)
  static const int env_seg = [] {
    const char *v = std::getenv("ESC_QUEUE_SEG");
    return v ? std::max(4, std::atoi(v)) : 0;
  }();
  static const int env_seg2 = [] {
    const char *v = std::getenv("ESC_QUEUE_SEG");
    const char *c = v ? std::strchr(v, ':') : nullptr;
    return c ? std::max(4, std::atoi(c + 1)) : 0;
  }();
  const int n_rec = (n_sph + 1) / 2;
  const bool merge_tris = n_tri > 0 && n_tri <= kQueueFewTris && n_rec > 0;
  if (n_tri > 0 && !merge_tris) cut(true, n_tri, 256, 1024, 2);
  const size_t first_sph = segs.size();
  // sphere segments of 768 pair records: measured on c4 (frame ms / lane efficiency) 256,256,512..:
  // 10.26 / 0.89, 768: 10.28 / 0.82, 1024: 10.40 / 0.79, 1536: 10.77 / 0.72 -- shorter segments
  // waste fewer lanes but re-read the survivors' rays more often; 768 keeps the speed with 7
  // launches and ~40 % less ray traffic than the short schedule
  if (n_rec > 0)
    cut(false, n_rec, env_seg ? env_seg : 768, env_seg2 ? env_seg2 : (env_seg ? env_seg : 768), 4);
  if (merge_tris) { // a floor and a light are not worth a pass over every ray of their own
    segs[first_sph + 0] = 0;
    segs[first_sph + 1] = n_tri;
  }
}

int render_shade_queue(esc_context *ctx, esc::RenderParams &p, int px, hipEvent_t between) {
  const size_t npx = (size_t)p.n_local_rows * p.W;
  if (npx > 0xfffffff0ull) {
    set_error("render: band too large for 32-bit pixel ids");
    return ESC_ERR_INVALID;
  }
  const size_t qcap = (npx + 63) / 64 * 64 + 64 * 4096; // ids per queue: every pixel + one partly
                                                         // filled chunk per workgroup
  const bool multi = p.n_lights > 1;
  // one allocation: rays | q0 | q1 | state
  const size_t off_rays = 0, off_q0 = off_rays + npx * sizeof(esc::ShadowRay),
               off_q1 = off_q0 + qcap * 4,
               off_state = off_q1 + qcap * 4, total = off_state + (multi ? npx * 16 : 0);
  int rc;
  if ((rc = ctx->frame.grow(ctx->d_sq, ctx->sq_bytes, total))) return rc;
  if (!ctx->n_cu) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    ctx->n_cu = std::max(1, prop.multiProcessorCount);
  }
  char *base = ctx->d_sq;
  // offsets are computed for THIS band (total <= the allocation)
  p.sq.rays = (esc::ShadowRay *)(base + off_rays);
  p.sq.q[0] = (uint32_t *)(base + off_q0);
  p.sq.q[1] = (uint32_t *)(base + off_q1);
  p.sq.state = multi ? (float *)(base + off_state) : nullptr;
  std::vector<int> segs;
  queue_segments(p.n_tri, p.n_sph, segs);
  const int n_segs = (int)segs.size() / 4;
  const size_t ctl_words = (size_t)p.n_lights * n_segs * 2;
  if ((rc = ctx->frame.grow(ctx->d_sq_ctl, ctx->sq_ctl_words, ctl_words))) return rc;
  p.sq.ctl = ctx->d_sq_ctl;
  HIP_TRY(hipMemsetAsync(ctx->d_sq_ctl, 0, ctl_words * 4, ctx->stream));
  int e = esc_launch_primary_only(&p, px, ctx->stream);
  if (e) {
    set_error(std::string("k_primary launch: ") + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  if (between) HIP_TRY(hipEventRecord(between, ctx->stream));
  // persistent-style grid of the segment kernels: 8 workgroups of 4 waves per CU fill every SIMD
  // (8 waves each); more would only queue behind them
  const int n_wg = std::min(4096, ctx->n_cu * 8);
  for (int li = 0; li < p.n_lights; li++) {
    e = esc_launch_shade_queue(&p, li, li == p.n_lights - 1, segs.data(), n_segs,
                               ctx->d_sq_ctl + (size_t)li * n_segs * 2, n_wg, ctx->stream);
    if (e) {
      set_error(std::string("shadow-queue kernel launch: ") + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  return ESC_OK;
}

// the one place a frame kernel is launched from: local row lr (ascending h) maps to image row
// h0 + (lr / strip_rows) * strip_step + lr % strip_rows
int render_local_rows(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t h0,
                      int32_t n_local_rows, int32_t strip_rows, int32_t strip_step,
                      const esc_render_options *opts, float *d_rgb_f32, uint8_t *d_rgb_u8) {
  if (!ctx->have_scene) {
    set_error("render: no scene uploaded");
    return ESC_ERR_INVALID;
  }
  if ((int64_t)W * H > 0x7fffffffLL) {
    set_error("render: W*H exceeds the reference's int pixel index (main.cpp:784)");
    return ESC_ERR_INVALID;
  }
  if (opts->face_mode == ESC_FACE_FIXED &&
      (opts->fixed_face < 0 || (ctx->n_lights > 0 && opts->fixed_face >= ctx->min_light_faces))) {
    // main.cpp:743-748 draws faceID in [0, light.face_index.size())
    set_error("render: fixed_face must be in [0, face count of the smallest light)");
    return ESC_ERR_INVALID;
  }
  if (opts->pixels_per_lane != 0 && opts->pixels_per_lane != 1 && opts->pixels_per_lane != 2 &&
      opts->pixels_per_lane != 4) {
    set_error("render: pixels_per_lane must be 0 (auto), 1, 2 or 4");
    return ESC_ERR_INVALID;
  }
  // a degenerate camera (lookfrom == lookat, zero aspect: NaN / inf basis vectors) would make
  // every ray NaN; the kernels' filters are written for finite inputs, so it is refused
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->lower_left_corner[k]) ||
        !std::isfinite(cam->horizontal[k]) || !std::isfinite(cam->vertical[k])) {
      set_error("render: camera is not finite (lookfrom == lookat, or a zero / NaN aspect?)");
      return ESC_ERR_INVALID;
    }
  // the kernels store d_rgb_f32 as floats; d_rgb_u8 is written byte by byte unless it is aligned itself
  if (((uintptr_t)d_rgb_f32) & 3u) {
    set_error("render: device pointers must be 4-byte aligned (d_rgb_u8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n_local_rows == 0) return ESC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  // ESC_STAGE_BVH culls with proven bounds only.  Its tree and bins are proven for spheres (box pads
  // from the discriminant's error bound) and for up to kTinyTris triangles (tested directly); the
  // boxes of a triangle MESH carry a heuristic pad, so a scene with more triangles is
  // served by the structure that is proven for them -- the tile / light lists over the group levels
  // of the default path -- unless the caller asks for the tree by name.
  int32_t eff_stage = opts->stage;
  if (eff_stage == ESC_STAGE_BVH && ctx->n_tri > esc::kTinyTris && !(opts->flags & ESC_RENDER_BVH_HEURISTIC_PADS)) {
    const char *e = std::getenv("ESC_BVH_TREE"); // =1: as if the flag were set (tests, tools, viewer)
    if (!(e && std::strcmp(e, "1") == 0)) eff_stage = ESC_STAGE_AUTO;
  }

  esc::RenderParams p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.origin, cam->origin, 12);
  std::memcpy(p.llc, cam->lower_left_corner, 12);
  std::memcpy(p.horizontal, cam->horizontal, 12);
  std::memcpy(p.vertical, cam->vertical, 12);
  p.W = W;
  p.H = H;
  p.h0 = h0;
  p.n_local_rows = n_local_rows;
  p.strip_rows = strip_rows;
  p.strip_step = strip_step;
  p.n_tri = ctx->n_tri;
  p.n_sph = ctx->n_sph;
  p.n_lights = ctx->n_lights;
  p.n_geom = ctx->n_geom;
  p.tri = ctx->d_tri;
  p.tri_p = ctx->d_tri_p;
  p.tri_n = ctx->d_tri_n;
  p.tri_face = ctx->d_tri_face;
  p.sph = ctx->d_sph;
  p.sph_p = ctx->d_sph_p;
  p.sph2 = ctx->d_sph2;
  p.sph_f = ctx->d_sph_f;
  p.sph2_f = ctx->d_sph2_f;
  bool linear_sweeps = false; // ESC_RENDER_INDEX_ORDER / ESC_GROUPS=0: the linear loops, untouched by any list
  {
    static const bool env_index = [] {
      const char *e = std::getenv("ESC_ORDER");
      return e && std::strcmp(e, "index") == 0;
    }();
    const bool index_order = env_index || (opts->flags & ESC_RENDER_INDEX_ORDER);
    p.sph2_ord = index_order ? nullptr : ctx->d_sph2_ord;
    p.sph2_f_ord = index_order ? nullptr : ctx->d_sph2_f_ord;
    static const bool env_nogroups = [] {
      const char *e = std::getenv("ESC_GROUPS");
      return e && std::strcmp(e, "0") == 0;
    }();
    p.sg = ctx->sg;
    p.tg = ctx->tg;
    if (index_order || env_nogroups)
      p.sg.n_grp = p.sg.n_sup = p.sg.n_hyp = p.tg.n_grp = p.tg.n_sup = p.tg.n_hyp = 0;
    linear_sweeps = index_order || env_nogroups;

  }
  p.tri_f = ctx->d_tri_f;
  p.tri_pf = ctx->d_tri_pf;
  p.tri2_pf = ctx->d_tri2_pf;
  p.tri2_f = ctx->d_tri2_f;
  p.shadow_rho_max = ctx->shadow_rho_max;
  std::memcpy(p.shadow_center, ctx->shadow_center, 12);
  std::memcpy(p.scene_lo, ctx->scene_lo, 12);
  std::memcpy(p.scene_hi, ctx->scene_hi, 12);
  {
    static const bool env_off = [] {
      const char *e = std::getenv("ESC_FILTER");
      return e && std::strcmp(e, "0") == 0;
    }();
    p.use_filter = (env_off || (opts->flags & ESC_RENDER_EXACT_ONLY)) ? 0 : 1;
  }
  p.sph_mat = ctx->d_sph_mat;
  p.mat = ctx->d_mat;
  p.lights = ctx->d_lights;
  p.light_points = ctx->d_light_points;
  p.shadows = opts->shadows ? 1 : 0;
  p.face_mode = opts->face_mode;
  p.fixed_face = opts->fixed_face;
  p.seed = opts->seed;
  p.out_f32 = d_rgb_f32;
  p.out_u8 = d_rgb_u8;
  p.counters = (opts->flags & ESC_RENDER_NO_COUNTERS) ? nullptr : ctx->d_counters;
  {
    const int rc = ctx->frame.grow(ctx->d_hits, ctx->hits_cap, (size_t)n_local_rows * W * 3);
    if (rc) return rc;
    const size_t plane = ctx->hits_cap / 3;
    p.hits.idx = ctx->d_hits;
    p.hits.t = reinterpret_cast<float *>(ctx->d_hits + plane);
    p.hits.v = reinterpret_cast<float *>(ctx->d_hits + 2 * plane);
  }

  if (!ctx->prepared || std::memcmp(ctx->prepared_origin, cam->origin, 12) != 0) {
    int e = esc_launch_prepare(&p, ctx->d_tri_p, ctx->d_tri_f, ctx->d_tri_pf, ctx->d_sph_p,
                               ctx->d_sph_f, &ctx->sg, &ctx->tg, ctx->stream);
    if (e) {
      set_error(std::string("k_prepare_primary launch: ") + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
    std::memcpy(ctx->prepared_origin, cam->origin, 12);
    ctx->prepared = true;
    ctx->epoch++;
  }
  // ---- k_frame's ray tables (rt_device.h RayTables): per camera frame and image size, whatever path
  // this call takes -- every frame k_frame renders finds them.  Rebuilt like the tables above: on this
  // stream, behind the frames that read the old entries, and ending the recorded frames.
  {
    esc_context::RayKey key;
    std::memset(&key, 0, sizeof(key));
    std::memcpy(key.cam, cam->lower_left_corner, 12);
    std::memcpy(key.cam + 3, cam->horizontal, 12);
    std::memcpy(key.cam + 6, cam->vertical, 12);
    key.W = W;
    key.H = H;
    if (!ctx->rays_valid || std::memcmp(&key, &ctx->ray_key, sizeof(key)) != 0) {
      ctx->rays_valid = false;
      int rc;
      if ((rc = ctx->frame.grow(ctx->d_ray_col, ctx->ray_col_cap, (size_t)W))) return rc;
      if ((rc = ctx->frame.grow(ctx->d_ray_row, ctx->ray_row_cap, (size_t)H))) return rc;
      int e = esc_launch_ray_tables(&p, ctx->d_ray_col, ctx->d_ray_row, ctx->stream);
      if (e) {
        set_error(std::string("k_prepare_ray_tables launch: ") + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
      ctx->ray_key = key;
      ctx->rays_valid = true;
      ctx->epoch++;
    }
  }
  // ---- tile lists of the primary pass (rt_lists.h): per camera and band, cached while both stand
  {
    static const bool env_nolists = [] {
      const char *e = std::getenv("ESC_LISTS");
      return e && std::strcmp(e, "0") == 0;
    }();
    const bool allowed = !env_nolists && !(opts->flags & ESC_RENDER_NO_TILE_LISTS) && p.use_filter &&
                         eff_stage != ESC_STAGE_LDS && eff_stage != ESC_STAGE_BVH && (h0 % 4) == 0;
    // a triangle table too small for groups, swept directly: one mask word per tile in tl.cnt instead
    // (rt_lists.h "Per-tile triangle masks"); switched with the lists.  Only the kernels with two pixels
    // per lane read them (primary_closest, PX == 2): a frame of 1 or 4 pixels per lane builds none.
    const bool px2 = opts->pixels_per_lane == 0 || opts->pixels_per_lane == 2;
    const bool want_masks = allowed && px2 && !linear_sweeps && p.n_tri > 0 && p.n_tri <= 32;
    const bool want = allowed && (p.sg.n_grp > 0 || p.tg.n_grp > 0 || want_masks);
    ctx->tri_masks_last = want_masks;
    if (want) {
      const int tiles_x = (W + 31) / 32, tile_rows = (n_local_rows + 3) / 4;
      const size_t n_tiles = (size_t)tiles_x * tile_rows;
      // headers and counts exist for both kinds; the slot arrays (kTileListCap ints per tile: 0.5 GB
      // for an 8K frame) only for the kinds this scene has
      const bool need_ids[2] = {p.sg.n_grp > 0, p.tg.n_grp > 0};
      const bool grow = n_tiles > ctx->list_tiles_cap || !ctx->sl.hdr;
      if (grow || (need_ids[0] && !ctx->sl.ids) || (need_ids[1] && !ctx->tl.ids)) {
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // an earlier frame may still read the old lists
        int rc;
        if (grow) {
          ctx->list_tiles_cap = 0;
          ctx->lists_valid = false;
          for (esc::TileLists *L : {&ctx->sl, &ctx->tl}) {
            if ((rc = ctx->frame.alloc(L->hdr, (size_t)esc::kTileHdrInts))) return rc;
            if ((rc = ctx->frame.alloc(L->cnt, n_tiles))) return rc;
            if ((rc = ctx->frame.release(L->ids))) return rc; // sized by the old capacity: allocated again below
          }
          if ((rc = ctx->frame.alloc(ctx->tl.esc, (size_t)esc::kTileEscCap))) return rc;
          ctx->list_tiles_cap = n_tiles;
        }
        int k = 0;
        for (esc::TileLists *L : {&ctx->sl, &ctx->tl}) {
          if (need_ids[k++] && !L->ids) {
            if ((rc = ctx->frame.alloc(L->ids, ctx->list_tiles_cap * esc::kTileListCap))) return rc;
            // slots past a count are read in whole batches of 4: zeros are valid slots
            HIP_TRY(hipMemsetAsync(L->ids, 0, ctx->list_tiles_cap * esc::kTileListCap * 4, ctx->stream));
            ctx->lists_valid = false;
          }
        }
      }
      esc_context::ListKey key;
      std::memset(&key, 0, sizeof(key));
      std::memcpy(key.cam, cam->origin, 12);
      std::memcpy(key.cam + 3, cam->lower_left_corner, 12);
      std::memcpy(key.cam + 6, cam->horizontal, 12);
      std::memcpy(key.cam + 9, cam->vertical, 12);
      key.W = W; key.H = H; key.h0 = h0; key.n_local_rows = n_local_rows;
      key.strip_rows = strip_rows; key.strip_step = strip_step;
      key.n_sg = p.sg.n_grp; key.n_tg = p.tg.n_grp;
      key.n_mask_tri = want_masks ? p.n_tri : 0;
      p.sl = ctx->sl;
      p.tl = ctx->tl;
      p.sl.tiles_x = p.tl.tiles_x = tiles_x;
      p.sl.tile_rows = p.tl.tile_rows = tile_rows;
      p.sl.enabled = p.sg.n_grp > 0;
      p.tl.enabled = p.tg.n_grp > 0;
      p.sl.masks = 0;
      p.tl.masks = want_masks ? 1 : 0;
      if (!ctx->lists_valid || std::memcmp(&key, &ctx->list_key, sizeof(key)) != 0) {
        for (const esc::TileLists *L : {&p.sl, &p.tl}) {
          HIP_TRY(hipMemsetAsync(L->hdr, 0, (size_t)esc::kTileHdrInts * 4, ctx->stream));
          HIP_TRY(hipMemsetAsync(L->cnt, 0, n_tiles * 4, ctx->stream));
          if (ctx->list_ids_stale && L->ids) // slots past a count are read in whole batches: keep them valid
            HIP_TRY(hipMemsetAsync(L->ids, 0, ctx->list_tiles_cap * esc::kTileListCap * 4, ctx->stream));
        }
        ctx->list_ids_stale = false;
        int e = esc_launch_tile_lists(&p, ctx->stream);
        if (e) {
          set_error(std::string("k_bin_*_groups launch: ") + hipGetErrorString((hipError_t)e));
          return ESC_ERR_HIP;
        }
        ctx->list_key = key;
        ctx->lists_valid = true;
        ctx->epoch++;
      }
    }
  }
  // ---- light lists of the shadow pass (rt_lists.h): per scene and sample point
  {
    static const bool env_nollists = [] {
      const char *e = std::getenv("ESC_LLISTS");
      return e && std::strcmp(e, "0") == 0;
    }();
    int n_listed = 0; // leading lights that offer ONE sample point this frame
    while (n_listed < std::min(ctx->n_lights, (int)esc::kLightListMax) &&
           (opts->face_mode == ESC_FACE_FIXED || ctx->h_lights[(size_t)n_listed].n_faces == 1))
      n_listed++;
    const bool want = !env_nollists && !(opts->flags & ESC_RENDER_NO_LIGHT_LISTS) && p.use_filter &&
                      p.shadows && (p.sg.n_grp > 0 || p.tg.n_grp > 0) && n_listed > 0 &&
                      eff_stage != ESC_STAGE_LDS && eff_stage != ESC_STAGE_BVH;
    if (want) {
      const int Rr = esc::kLightListRes;
      const size_t cells = (size_t)n_listed * 6 * Rr * Rr;
      if (n_listed > ctx->ll_alloc_lights) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int rc;
        ctx->ll_alloc_lights = 0;
        for (esc::LightLists *L : {&ctx->ll, &ctx->lt}) {
          if ((rc = ctx->frame.alloc(L->hdr, (size_t)n_listed * 6 * esc::kTileHdrInts))) return rc;
          if ((rc = ctx->frame.alloc(L->cnt, cells))) return rc;
          if ((rc = ctx->frame.alloc(L->ids, cells * esc::kLightListCap))) return rc;
        }
        if ((rc = ctx->frame.alloc(ctx->lt.esc, (size_t)n_listed * esc::kLightEscCap))) return rc;
        if ((rc = ctx->frame.alloc(ctx->ll.pk_cell, cells))) return rc;
        if (!ctx->ll.pk_total) { // steps, refused cells, and k_frame's tripwire (rt_device.h): zero once
          if ((rc = ctx->frame.alloc(ctx->ll.pk_total, 3))) return rc;
          HIP_TRY(hipMemsetAsync(ctx->ll.pk_total, 0, 12, ctx->stream));
        }
        ctx->ll_alloc_lights = n_listed;
        ctx->ll_valid = false;
      }
      for (esc::LightLists *src : {&ctx->ll, &ctx->lt}) {
        esc::LightLists L = *src;
        L.n_listed = n_listed;
        L.R = Rr;
        L.enabled = (src == &ctx->ll) ? (p.sg.n_grp > 0) : (p.tg.n_grp > 0);
        for (int li = 0; li < n_listed; li++)
          L.point[li] = ctx->h_lights[(size_t)li].first_point +
                        (opts->face_mode == ESC_FACE_FIXED ? opts->fixed_face : 0);
        (src == &ctx->ll ? p.ll : p.lt) = L;
      }
      const bool rebuild = !ctx->ll_valid || ctx->ll_face_mode != opts->face_mode ||
                           (opts->face_mode == ESC_FACE_FIXED && ctx->ll_fixed_face != opts->fixed_face) ||
                           ctx->ll.n_listed != n_listed;
      if (rebuild) {
        for (const esc::LightLists *L : {&p.ll, &p.lt}) {
          HIP_TRY(hipMemsetAsync(L->hdr, 0, (size_t)n_listed * 6 * esc::kTileHdrInts * 4, ctx->stream));
          HIP_TRY(hipMemsetAsync(L->cnt, 0, cells * 4, ctx->stream));
          // spare slots of a cell are read in whole batches of 4: zeros are valid pair records
          HIP_TRY(hipMemsetAsync(L->ids, 0, cells * esc::kLightListCap * 4, ctx->stream));
        }
        int e = esc_launch_light_lists(&p, ctx->stream);
        if (e) {
          set_error(std::string("k_bin_light_* launch: ") + hipGetErrorString((hipError_t)e));
          return ESC_ERR_HIP;
        }
        // the packed form of the sphere lists: count, size the stream exactly (one read-back per scene
        // and sample point; this path never runs inside a capture), fill
        ctx->ll_pk_steps = -1;
        ctx->ll_complete = false;
        if (p.ll.enabled) {
          HIP_TRY(hipMemsetAsync(p.ll.pk_total, 0, 8, ctx->stream));
          if ((e = esc_launch_light_pack(&p, 0, ctx->stream))) {
            set_error(std::string("k_pack_light_cells launch: ") + hipGetErrorString((hipError_t)e));
            return ESC_ERR_HIP;
          }
          HIP_TRY(hipStreamSynchronize(ctx->stream));
          int32_t total[2] = {0, 0}; // steps; cells and faces the sweep would refuse
          HIP_TRY(hipMemcpy(total, p.ll.pk_total, 8, hipMemcpyDeviceToHost));
          const int32_t steps = total[0];
          if (steps < 0) {
            set_error("k_pack_light_cells: the packed light lists do not fit 2^31 steps");
            return ESC_ERR_HIP;
          }
          if (!ctx->ll.pk_rec || (size_t)steps > ctx->ll_pk_steps_cap) {
            int rc;
            ctx->ll_pk_steps_cap = 0;
            if ((rc = ctx->frame.alloc(ctx->ll.pk_rec, 2 * (size_t)steps + 2))) return rc;
            if ((rc = ctx->frame.alloc(ctx->ll.pk_pos, 4 * (size_t)steps + 4))) return rc;
            ctx->ll_pk_steps_cap = (size_t)steps;
            p.ll.pk_rec = ctx->ll.pk_rec;
            p.ll.pk_pos = ctx->ll.pk_pos;
          }
          // (the spare step at the end of the stream, and whatever a shorter stream leaves: pad halves
          // need no writing -- nothing read past a cell's steps is ever tested)
          HIP_TRY(hipMemsetAsync(p.ll.pk_rec + 2 * (size_t)steps, 0, 2 * sizeof(esc::DevSphPair), ctx->stream));
          if ((e = esc_launch_light_pack(&p, 1, ctx->stream))) {
            set_error(std::string("k_pack_light_cells launch: ") + hipGetErrorString((hipError_t)e));
            return ESC_ERR_HIP;
          }
          ctx->ll_pk_steps = steps;
          ctx->ll_complete = total[1] == 0;
        }
        ctx->ll.n_listed = ctx->lt.n_listed = n_listed;
        ctx->ll.R = ctx->lt.R = Rr;
        std::memcpy(ctx->ll.point, p.ll.point, sizeof(p.ll.point)); // (for esc_light_list_read)
        std::memcpy(ctx->lt.point, p.lt.point, sizeof(p.lt.point));
        ctx->ll_face_mode = opts->face_mode;
        ctx->ll_fixed_face = opts->fixed_face;
        ctx->ll_valid = true;
        ctx->epoch++;
      }
      // the A/B switch: the consumer sweeps the id lists when it gets no packed cells
      if ((opts->flags & ESC_RENDER_NO_PACKED_LIGHT_LISTS) || !p.ll.enabled || ctx->ll_pk_steps < 0) p.ll.pk_cell = nullptr;
    }
  }
  int stage = (eff_stage == ESC_STAGE_LDS) ? 2 : 1; // AUTO -> SMEM (measured)
  // pixels per work-item of the PRIMARY pass; AUTO = 2 (measured)
  int px = opts->pixels_per_lane ? opts->pixels_per_lane : 2;
  if (eff_stage == ESC_STAGE_BVH) {
    if (!ctx->accel_valid || !ctx->accel_ob.contains(cam->origin)) {
      int rc = build_accel_device(ctx, cam->origin);
      if (rc) return rc;
    }
    if (!ctx->accel_prepared || std::memcmp(ctx->accel_prepared_origin, cam->origin, 12) != 0) {
      int e = esc_launch_prepare_bvh(
          reinterpret_cast<const esc::DevTri *>(ctx->d_bvh_tri_blocks),
          reinterpret_cast<esc::DevTriP *>(ctx->d_bvh_tri_blocks_p),
          ctx->accel_info.tri_blocks * esc::kTriBlock,
          reinterpret_cast<const esc::DevSph *>(ctx->d_bvh_sph_blocks),
          reinterpret_cast<esc::DevSphP *>(ctx->d_bvh_sph_blocks_p),
          ctx->accel_info.sph_blocks * esc::kSphBlock, cam->origin[0], cam->origin[1],
          cam->origin[2], ctx->stream);
      if (e) {
        set_error(std::string("k_prepare_bvh launch: ") + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
      std::memcpy(ctx->accel_prepared_origin, cam->origin, 12);
      ctx->accel_prepared = true;
      ctx->epoch++;
    }
    p.bvh_tri = esc::BvhRef{ctx->d_bvh_tri_nodes, ctx->d_bvh_tri_blocks, ctx->d_bvh_tri_blocks_p,
                            ctx->d_bvh_tri_order, ctx->accel_info.tri_root, 0};
    p.bvh_sph = esc::BvhRef{ctx->d_bvh_sph_nodes, ctx->d_bvh_sph_blocks, ctx->d_bvh_sph_blocks_p,
                            ctx->d_bvh_sph_order, ctx->accel_info.sph_root, 0};
    // screen-space bins for the primary pass: rebuilt every frame on the stream (they depend on
    // the camera), sized for the image
    const char *no_bins = std::getenv("ESC_BVH_BINS");
    if (!(no_bins && std::strcmp(no_bins, "0") == 0)) {
      const int tiles_x = (W + 31) / 32, groups_y = (H + esc::kTileH - 1) / esc::kTileH;
      const size_t n_bins = (size_t)tiles_x * groups_y;
      if (tiles_x != ctx->bin_tiles_x || groups_y != ctx->bin_groups_y) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int rc;
        ctx->bin_tiles_x = ctx->bin_groups_y = 0;
        if ((rc = ctx->frame.alloc(ctx->d_bin_hdr, esc::kBinHdrInts + 2 * n_bins))) return rc;
        if ((rc = ctx->frame.alloc(ctx->d_bin_tri_ids, n_bins * esc::kBinCap))) return rc;
        if ((rc = ctx->frame.alloc(ctx->d_bin_sph_ids, n_bins * esc::kBinCap))) return rc;
        // ids start as zeros: a slot past a bin's count must always name a valid primitive
        HIP_TRY(hipMemsetAsync(ctx->d_bin_tri_ids, 0, n_bins * esc::kBinCap * 4, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->d_bin_sph_ids, 0, n_bins * esc::kBinCap * 4, ctx->stream));
        ctx->bin_tiles_x = tiles_x;
        ctx->bin_groups_y = groups_y;
      }
      p.bins = esc::BinGrid{ctx->d_bin_hdr, ctx->d_bin_tri_ids, ctx->d_bin_sph_ids, tiles_x,
                            groups_y};
      p.lbins = ctx->lbins;
      HIP_TRY(hipMemsetAsync(ctx->d_bin_hdr, 0, (esc::kBinHdrInts + 2 * n_bins) * 4, ctx->stream));
      int e = esc_launch_bin_primary(&p, ctx->d_tri_boxes, ctx->d_sph_boxes, ctx->stream);
      if (e) {
        set_error(std::string("k_bin_primary launch: ") + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
    }
    stage = 3;
    px = 1; // a wave walks the tree with its 64 rays
  }
  const bool timed = (opts->flags & ESC_RENDER_TIME_KERNELS) != 0;
  ctx->ev_valid = false;
  ctx->last_frame_kernel = 0;
  if (timed) {
    for (auto &ev : ctx->ev)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
  }
  int e;
  // Brute force with shadows over a long primitive list: the queue form of the shadow pass
  // (global compaction of undecided rays between segments).  Short lists keep the fused k_shade
  // (its per-workgroup re-packing costs no extra launches); $ESC_SHADE=wg|queue overrides.
  static const int shade_env = [] {
    const char *v = std::getenv("ESC_SHADE");
    return !v ? 0 : (std::strcmp(v, "wg") == 0 ? 1 : (std::strcmp(v, "queue") == 0 ? 2 : 0));
  }();
  const int want = (opts->flags & ESC_RENDER_SHADE_QUEUE) ? 2
                   : (opts->flags & ESC_RENDER_SHADE_FUSED) ? 1 : shade_env;
  // Shadow rays sweep the primitive GROUPS (rt_device.h SphGroups / TriGroups) in the fused form
  // only -- the last light in any order, earlier lights in "first occluder" mode as long as a
  // table is one segment (2^20 records) -- so a grouped table counts as nothing here.
  const bool sph_grouped = p.use_filter && p.sg.n_grp > 0 &&
                           (p.n_lights == 1 || (int64_t)p.sg.n_grp * (esc::kSphGroup / 2) <= (1 << 20));
  const bool tri_grouped = p.use_filter && p.tg.n_grp > 0 &&
                           (p.n_lights == 1 || (int64_t)p.tg.n_grp * esc::kTriGroup <= (1 << 20));
  const int64_t eff_sph = sph_grouped ? 0 : p.n_sph;
  const int64_t eff_tri = tri_grouped ? 0 : p.n_tri;
  const bool queue_form =
      stage == 1 && p.shadows && p.n_lights > 0 && want != 1 &&
      (want == 2 || eff_stage == ESC_STAGE_AUTO) &&
      (want == 2 || (eff_tri + eff_sph >= kQueueMinPrims &&
                     (int64_t)n_local_rows * W >= kQueueMinPixels));
  if (queue_form) {
    int rc = render_shade_queue(ctx, p, px, timed ? ctx->ev[1] : nullptr);
    if (rc) return rc;
    e = 0;
  } else {
    static const bool env_two = [] {
      const char *v = std::getenv("ESC_FRAME");
      return v && std::strcmp(v, "2") == 0;
    }();
    // k_frame without the vote and the fallback sweep (rt_kernels.hip "SURE"): only when no wave can
    // be refused -- complete packed sphere lists, one light (quirk S3 starts a later light's ray
    // wherever the previous light's t left it), and a camera whose primary hits all give shadow
    // origins inside the box (asked once per camera origin and scene).  The launch code adds what it
    // can see in p: every light covered, no triangle groups, the packed instantiation.
    static const bool env_vote = [] {
      const char *v = std::getenv("ESC_SURE");
      return v && std::strcmp(v, "0") == 0;
    }();
    if (!env_vote && !(opts->flags & ESC_RENDER_VOTE) && p.shadows && p.ll.enabled && p.ll.pk_cell &&
        ctx->ll_valid && ctx->ll_complete && ctx->n_lights == 1 && p.tg.n_grp == 0) {
      if (!ctx->sure_known || std::memcmp(ctx->sure_origin, cam->origin, 12) != 0) {
        ctx->sure_inside = esc::shadow_origins_inside(cam->origin, ctx->scene_lo, ctx->scene_hi, ctx->h_tri.data(),
                                                      ctx->h_tri.size(), ctx->n_lights);
        std::memcpy(ctx->sure_origin, cam->origin, 12);
        ctx->sure_known = true;
      }
      p.sure = ctx->sure_inside ? 1 : 0;
    }
    int which = 0;
    const esc::RayTables rays{ctx->d_ray_col, ctx->d_ray_row};
    e = esc_launch_render(&p, &rays, stage, px, ctx->stream, timed ? ctx->ev[1] : nullptr,
                          (env_two || (opts->flags & ESC_RENDER_TWO_KERNELS)) ? 1 : 0, &which);
    ctx->last_frame_kernel = which;
  }
  if (timed && !e) {
    HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
    ctx->ev_valid = true;
  }
  if (e) {
    set_error(std::string("frame kernel launch (k_primary / k_shade): ") + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

} // namespace

extern "C" {

int esc_render_rows(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                    int32_t row_begin, int32_t row_end, const esc_render_options *opts,
                    float *d_rgb_f32, uint8_t *d_rgb_u8) {
  if (!ctx || !cam || !opts) {
    set_error("esc_render_rows: bad argument");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2 || row_begin < 0 || row_end > H || row_begin > row_end) {
    // W-1 and H-1 are divisors at main.cpp:709-710
    set_error("esc_render_rows: need W,H >= 2 and 0 <= row_begin <= row_end <= H");
    return ESC_ERR_INVALID;
  }
  // one "strip" taller than any image: lr / strip_rows == 0
  return render_local_rows(ctx, cam, W, H, row_begin, row_end - row_begin, 1 << 30, 0, opts,
                           d_rgb_f32, d_rgb_u8);
}

int esc_strip_local_rows(int32_t H, int32_t strip_rows, int32_t first_strip,
                         int32_t strip_stride) {
  if (H < 1 || strip_rows < 8 || strip_rows % 8 != 0 || first_strip < 0 || strip_stride < 1) {
    set_error("esc_strip_local_rows: need H >= 1, strip_rows a positive multiple of 8, "
              "first_strip >= 0, strip_stride >= 1");
    return ESC_ERR_INVALID;
  }
  const int n_strips = (H + strip_rows - 1) / strip_rows;
  int64_t rows = 0;
  for (int k = first_strip; k < n_strips; k += strip_stride)
    rows += std::min(strip_rows, H - k * strip_rows);
  return (int)rows;
}

int esc_render_strips(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                      int32_t strip_rows, int32_t first_strip, int32_t strip_stride,
                      const esc_render_options *opts, float *d_rgb_f32, uint8_t *d_rgb_u8) {
  if (!ctx || !cam || !opts) {
    set_error("esc_render_strips: bad argument");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error("esc_render_strips: need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  const int rows = esc_strip_local_rows(H, strip_rows, first_strip, strip_stride);
  if (rows < 0) return rows;
  return render_local_rows(ctx, cam, W, H, first_strip * strip_rows, rows, strip_rows,
                           strip_stride * strip_rows, opts, d_rgb_f32, d_rgb_u8);
}

struct esc_frame {
  esc_context *ctx = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint64_t epoch = 0;
};

int esc_frame_record(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t strip_rows,
                     int32_t first_strip, int32_t strip_stride, const esc_render_options *opts,
                     float *d_rgb_f32, uint8_t *d_rgb_u8, esc_frame **out) {
  if (!ctx || !cam || !opts || !out) {
    set_error("esc_frame_record: bad argument");
    return ESC_ERR_INVALID;
  }
  if (opts->flags & ESC_RENDER_TIME_KERNELS) {
    set_error("esc_frame_record: ESC_RENDER_TIME_KERNELS records events between the kernels and "
              "cannot be part of a recorded frame");
    return ESC_ERR_INVALID;
  }
  // one plain frame first: it builds everything the frame's kernels read (per-camera tables, the
  // lists, scratch buffers) -- none of that may happen inside a stream capture
  int rc = esc_render_strips(ctx, cam, W, H, strip_rows, first_strip, strip_stride, opts, d_rgb_f32,
                             d_rgb_u8);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t epoch = ctx->epoch;
  esc_frame *f = new (std::nothrow) esc_frame();
  if (!f) return ESC_ERR_NOMEM;
  f->ctx = ctx;
  hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    set_error(std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    delete f;
    return ESC_ERR_HIP;
  }
  const unsigned refused = ctx->frame.refused();
  ctx->capturing = true;
  rc = esc_render_strips(ctx, cam, W, H, strip_rows, first_strip, strip_stride, opts, d_rgb_f32,
                         d_rgb_u8);
  ctx->capturing = false;
  e = hipStreamEndCapture(ctx->stream, &f->graph);
  // frame memory refuses to be freed or allocated inside the capture: the render then failed for that
  if (ctx->frame.refused() != refused || (rc == ESC_OK && ctx->epoch != epoch)) {
    set_error("esc_frame_record: device state was rebuilt during the capture");
    rc = ESC_ERR_HIP;
  } else if (rc == ESC_OK && e != hipSuccess) {
    set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    rc = ESC_ERR_HIP;
  }
  if (rc == ESC_OK) {
    e = hipGraphInstantiate(&f->exec, f->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
      rc = ESC_ERR_HIP;
    }
  }
  if (rc != ESC_OK) {
    if (f->graph) (void)hipGraphDestroy(f->graph);
    delete f;
    return rc;
  }
  f->epoch = epoch;
  *out = f;
  return ESC_OK;
}

int esc_frame_valid(const esc_frame *f) { return (f && f->exec && f->ctx->epoch == f->epoch) ? 1 : 0; }

int esc_frame_launch(esc_frame *f) {
  if (!f || !f->exec) {
    set_error("esc_frame_launch: bad argument");
    return ESC_ERR_INVALID;
  }
  if (!esc_frame_valid(f)) {
    set_error("esc_frame_launch: the context rendered another camera, size or scene since this "
              "frame was recorded (its kernels would read rebuilt tables): record it again");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipGraphLaunch(f->exec, f->ctx->stream));
  return ESC_OK;
}

void esc_frame_destroy(esc_frame *f) {
  if (!f) return;
  if (f->exec) (void)hipGraphExecDestroy(f->exec);
  if (f->graph) (void)hipGraphDestroy(f->graph);
  delete f;
}

int esc_assemble_strips(esc_context *ctx, const void *d_gathered, int32_t n_ranks,
                        size_t rank_pitch_bytes, int32_t W, int32_t H, int32_t strip_rows,
                        int32_t bytes_per_pixel, void *d_frame) {
  if (!ctx || !d_gathered || !d_frame || n_ranks < 1 || W < 1 || H < 1 || strip_rows < 1 ||
      bytes_per_pixel < 1) {
    set_error("esc_assemble_strips: bad argument");
    return ESC_ERR_INVALID;
  }
  // fp32 pixels (any pixel size that is a multiple of 4 bytes) are floats to whoever reads the frame
  if (bytes_per_pixel % 4 == 0 && ((((uintptr_t)d_gathered) | ((uintptr_t)d_frame)) & 3u)) {
    set_error("esc_assemble_strips: device pointers must be 4-byte aligned (byte pixels excepted)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  int e = esc_launch_assemble(d_gathered, d_frame, rank_pitch_bytes, n_ranks, H, strip_rows,
                              (size_t)W * bytes_per_pixel, ctx->stream);
  if (e) {
    set_error(std::string("k_assemble_strips launch: ") + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_tri_group_record(const float *v0e1e2, int32_t count, float record[12]) {
  if (!v0e1e2 || !record || count <= 0) {
    set_error("esc_tri_group_record: bad argument");
    return ESC_ERR_INVALID;
  }
  std::vector<esc::DevTri> tri((size_t)count);
  std::vector<int32_t> order((size_t)count);
  for (int32_t i = 0; i < count; i++) {
    std::memset(&tri[(size_t)i], 0, sizeof(esc::DevTri));
    std::memcpy(tri[(size_t)i].v0, v0e1e2 + 9 * (size_t)i, 12);
    std::memcpy(tri[(size_t)i].e1, v0e1e2 + 9 * (size_t)i + 3, 12);
    std::memcpy(tri[(size_t)i].e2, v0e1e2 + 9 * (size_t)i + 6, 12);
    order[(size_t)i] = i;
  }
  const esc::DevTriGroup g = esc::tri_group_bounds(tri, order.data(), count);
  static_assert(offsetof(esc::DevTriGroup, slack) == 48, "the 12 floats of the record come first");
  std::memcpy(record, &g, 48);
  return ESC_OK;
}

int esc_sphere_group_record(const float *cxyzr2, int32_t count, float record[4]) {
  if (!cxyzr2 || !record || count <= 0) {
    set_error("esc_sphere_group_record: bad argument");
    return ESC_ERR_INVALID;
  }
  std::vector<esc::DevSph> sph((size_t)count);
  std::vector<int32_t> order((size_t)count);
  for (int32_t i = 0; i < count; i++) {
    std::memcpy(&sph[(size_t)i], cxyzr2 + 4 * (size_t)i, 16);
    order[(size_t)i] = i;
  }
  const esc::DevSphGroup g = esc::group_bounds(sph, order.data(), count);
  std::memcpy(record, &g, 16);
  return ESC_OK;
}

namespace {
void camera_params(const esc_camera *cam, int32_t W, int32_t H, esc::RenderParams &p) {
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.origin, cam->origin, 12);
  std::memcpy(p.llc, cam->lower_left_corner, 12);
  std::memcpy(p.horizontal, cam->horizontal, 12);
  std::memcpy(p.vertical, cam->vertical, 12);
  p.W = W;
  p.H = H;
}
} // namespace

int esc_tile_list_counts(esc_context *ctx, int32_t which, int32_t hdr[8], int32_t *counts,
                         size_t capacity) {
  if (!ctx || !hdr || which < 0 || which > 3) {
    set_error("esc_tile_list_counts: bad argument");
    return ESC_ERR_INVALID;
  }
  if (which >= 2) { // the light lists (2: sphere pairs, 3: triangle pairs): cells of every listed light and face
    const esc::LightLists &LLs = which == 2 ? ctx->ll : ctx->lt;
    if (!ctx->ll_valid || !LLs.hdr || (which == 2 ? ctx->sg.n_grp : ctx->tg.n_grp) == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int Rr = LLs.R, n_faces = LLs.n_listed * 6;
    int32_t glob_max = 0, n_esc = 0, off = 0;
    for (int f = 0; f < n_faces; f++) {
      int32_t g[3] = {0, 0, 0};
      HIP_TRY(hipMemcpy(g, LLs.hdr + (size_t)f * esc::kTileHdrInts, 12, hipMemcpyDeviceToHost));
      glob_max = std::max(glob_max, g[0]);
      n_esc += g[1]; // (kept on face 0 of each light)
      off |= g[2];
    }
    const int32_t out[8] = {glob_max, n_esc, off, Rr, n_faces * Rr, esc::kLightListCap, esc::kTileGlobalCap, 0};
    std::memcpy(hdr, out, sizeof(out));
    const size_t n_cells = (size_t)n_faces * Rr * Rr;
    if (counts)
      HIP_TRY(hipMemcpy(counts, LLs.cnt, std::min(capacity, n_cells) * 4, hipMemcpyDeviceToHost));
    return (int)n_cells;
  }
  const esc::TileLists &L = which ? ctx->tl : ctx->sl;
  const int n_groups = which ? ctx->list_key.n_tg : ctx->list_key.n_sg;
  if (!ctx->lists_valid || !L.hdr || n_groups == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int32_t h[3];
  HIP_TRY(hipMemcpy(h, L.hdr, sizeof(h), hipMemcpyDeviceToHost));
  const int tiles_x = (ctx->list_key.W + 31) / 32, tile_rows = (ctx->list_key.n_local_rows + 3) / 4;
  const int32_t out[8] = {h[0], h[1], h[2], tiles_x, tile_rows, esc::kTileListCap, esc::kTileGlobalCap, 0};
  std::memcpy(hdr, out, sizeof(out));
  const size_t n_tiles = (size_t)tiles_x * tile_rows;
  if (counts)
    HIP_TRY(hipMemcpy(counts, L.cnt, std::min(capacity, n_tiles) * 4, hipMemcpyDeviceToHost));
  return (int)n_tiles;
}

int esc_tile_list_ids(esc_context *ctx, int32_t which, int64_t index, int32_t *ids, int32_t capacity) {
  if (!ctx || !ids || which < 0 || which > 3 || index < -1 || (index == -1 && which >= 2) || capacity < 1) {
    set_error("esc_tile_list_ids: bad argument");
    return ESC_ERR_INVALID;
  }
  if (index == -1) { // the global list of the kind: hdr[0] appended, hdr[8..) the ids
    const esc::TileLists &L = which ? ctx->tl : ctx->sl;
    if (!ctx->lists_valid || !L.hdr) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int32_t c = 0;
    HIP_TRY(hipMemcpy(&c, L.hdr, 4, hipMemcpyDeviceToHost));
    const int m = std::min(std::min(c, (int32_t)esc::kTileGlobalCap), capacity);
    if (m > 0) HIP_TRY(hipMemcpy(ids, L.hdr + 8, (size_t)m * 4, hipMemcpyDeviceToHost));
    return c;
  }
  const int32_t *d_ids = nullptr, *d_cnt = nullptr;
  int cap = 0;
  int64_t n = 0;
  if (which < 2) {
    const esc::TileLists &L = which ? ctx->tl : ctx->sl;
    if (!ctx->lists_valid || !L.hdr || !L.ids) return 0;
    d_ids = L.ids; d_cnt = L.cnt; cap = esc::kTileListCap;
    n = (int64_t)((ctx->list_key.W + 31) / 32) * ((ctx->list_key.n_local_rows + 3) / 4);
  } else {
    const esc::LightLists &L = which == 2 ? ctx->ll : ctx->lt;
    if (!ctx->ll_valid || !L.hdr) return 0;
    d_ids = L.ids; d_cnt = L.cnt; cap = esc::kLightListCap;
    n = (int64_t)L.n_listed * 6 * L.R * L.R;
  }
  if (index >= n) {
    set_error("esc_tile_list_ids: index out of range");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int32_t c = 0;
  HIP_TRY(hipMemcpy(&c, d_cnt + index, 4, hipMemcpyDeviceToHost));
  const int m = std::min(std::min(c, cap), capacity);
  if (m > 0) HIP_TRY(hipMemcpy(ids, d_ids + index * cap, (size_t)m * 4, hipMemcpyDeviceToHost));
  return c;
}

int esc_tile_tri_masks(esc_context *ctx, int32_t info[8], uint32_t *masks, size_t capacity) {
  if (!ctx || !info) {
    set_error("esc_tile_tri_masks: bad argument");
    return ESC_ERR_INVALID;
  }
  const esc::TileLists &L = ctx->tl;
  if (!ctx->tri_masks_last || !ctx->lists_valid || !L.hdr || !L.cnt || ctx->list_key.n_mask_tri <= 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int32_t h[5];
  HIP_TRY(hipMemcpy(h, L.hdr, sizeof(h), hipMemcpyDeviceToHost));
  const int tiles_x = (ctx->list_key.W + 31) / 32, tile_rows = (ctx->list_key.n_local_rows + 3) / 4;
  const int32_t out[8] = {h[2], h[4], tiles_x, tile_rows, ctx->list_key.n_mask_tri, 0, 0, 0};
  std::memcpy(info, out, sizeof(out));
  const size_t n_tiles = (size_t)tiles_x * tile_rows;
  if (masks) HIP_TRY(hipMemcpy(masks, L.cnt, std::min(capacity, n_tiles) * 4, hipMemcpyDeviceToHost));
  return (int)n_tiles;
}

int esc_light_list_read(esc_context *ctx, int32_t which, int32_t info[8], int32_t *face_counts,
                        int32_t *face_ids, int64_t first_cell, int64_t n_cells, int32_t *cell_ids) {
  if (!ctx || !info || (which != 2 && which != 3) || first_cell < 0 || n_cells < 0) {
    set_error("esc_light_list_read: bad argument");
    return ESC_ERR_INVALID;
  }
  const esc::LightLists &L = which == 2 ? ctx->ll : ctx->lt;
  if (!ctx->ll_valid || !L.hdr || !L.cnt || !L.ids || (which == 2 ? ctx->sg.n_grp : ctx->tg.n_grp) == 0) return 0;
  const int n_faces = L.n_listed * 6;
  const int64_t total = (int64_t)n_faces * L.R * L.R;
  if (first_cell > total || n_cells > total - first_cell) {
    set_error("esc_light_list_read: cells out of range");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int32_t out[8] = {L.n_listed, L.R, esc::kLightListCap, esc::kTileGlobalCap,
                          L.point[0], L.point[1], L.point[2], L.point[3]};
  std::memcpy(info, out, sizeof(out));
  if (face_counts || face_ids) {
    std::vector<int32_t> hdr((size_t)n_faces * esc::kTileHdrInts);
    HIP_TRY(hipMemcpy(hdr.data(), L.hdr, hdr.size() * 4, hipMemcpyDeviceToHost));
    for (int f = 0; f < n_faces; f++) {
      const int32_t *h = &hdr[(size_t)f * esc::kTileHdrInts];
      if (face_counts) face_counts[f] = h[0];
      if (face_ids) {
        const int m = std::max(0, std::min(h[0], (int32_t)esc::kTileGlobalCap));
        for (int k = 0; k < esc::kTileGlobalCap; k++)
          face_ids[(size_t)f * esc::kTileGlobalCap + k] = k < m ? h[8 + k] : -1;
      }
    }
  }
  if (cell_ids && n_cells > 0) {
    std::vector<int32_t> cnt((size_t)n_cells);
    HIP_TRY(hipMemcpy(cnt.data(), L.cnt + first_cell, (size_t)n_cells * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cell_ids, L.ids + first_cell * esc::kLightListCap,
                      (size_t)n_cells * esc::kLightListCap * 4, hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < n_cells; c++) // slots past a cell's count hold stale (valid) records: not stored ids
      for (int k = std::max(0, std::min(cnt[(size_t)c], (int32_t)esc::kLightListCap)); k < esc::kLightListCap; k++)
        cell_ids[(size_t)c * esc::kLightListCap + k] = -1;
  }
  return (int)total;
}

int esc_light_list_packed_read(esc_context *ctx, int32_t info[8], int64_t first_cell, int64_t n_cells,
                               int32_t *steps, int32_t *slots) {
  if (!ctx || !info || first_cell < 0 || n_cells < 0) {
    set_error("esc_light_list_packed_read: bad argument");
    return ESC_ERR_INVALID;
  }
  const esc::LightLists &L = ctx->ll;
  if (!ctx->ll_valid || !L.hdr || !L.pk_cell || !L.pk_pos || ctx->ll_pk_steps < 0 || ctx->sg.n_grp == 0) return 0;
  const int64_t total = (int64_t)L.n_listed * 6 * L.R * L.R;
  if (first_cell > total || n_cells > total - first_cell) {
    set_error("esc_light_list_packed_read: cells out of range");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int32_t per_cell = 2 * esc::kLightListCap;
  const int32_t out[8] = {L.n_listed, L.R, per_cell, 4, ctx->ll_pk_steps, 0, 0, 0};
  std::memcpy(info, out, sizeof(out));
  if ((steps || slots) && n_cells > 0) {
    std::vector<esc::LightCell> cells((size_t)n_cells);
    HIP_TRY(hipMemcpy(cells.data(), L.pk_cell + first_cell, (size_t)n_cells * sizeof(esc::LightCell),
                      hipMemcpyDeviceToHost));
    std::vector<int32_t> pos;
    if (slots && ctx->ll_pk_steps > 0) {
      pos.resize(4 * (size_t)ctx->ll_pk_steps);
      HIP_TRY(hipMemcpy(pos.data(), L.pk_pos, pos.size() * 4, hipMemcpyDeviceToHost));
    }
    for (int64_t c = 0; c < n_cells; c++) {
      const esc::LightCell ce = cells[(size_t)c];
      if (steps) steps[c] = ce.n_steps < 0 ? -1 : ce.n_steps;
      if (!slots) continue;
      int32_t *row = slots + (size_t)c * per_cell;
      const bool ok = ce.n_steps > 0 && ce.offset >= 0 && 4 * (int64_t)ce.n_steps <= per_cell &&
                      (int64_t)ce.offset + ce.n_steps <= (int64_t)ctx->ll_pk_steps;
      const int m = ok ? 4 * ce.n_steps : 0;
      for (int k = 0; k < m; k++) row[k] = pos[4 * (size_t)ce.offset + k];
      for (int k = m; k < per_cell; k++) row[k] = -1;
    }
  }
  return (int)total;
}

int esc_tile_rect(const esc_camera *cam, int32_t W, int32_t H, const float centre[3], double radius,
                  int32_t rect[4]) {
  if (!cam || !centre || !rect || W < 2 || H < 2 || !(radius > 0.0)) {
    set_error("esc_tile_rect: bad argument");
    return ESC_ERR_INVALID;
  }
  esc::RenderParams p;
  camera_params(cam, W, H, p);
  const esc::CamD c = esc::cam_frame(p);
  if (!c.ok) return 0;
  const double rel[3] = {(double)centre[0] - c.o[0], (double)centre[1] - c.o[1], (double)centre[2] - c.o[2]};
  int w0 = 0, w1 = -1, h0 = 0, h1 = -1;
  const int st = esc::sphere_pixel_rect(c, W, H, rel, radius, w0, w1, h0, h1);
  rect[0] = w0; rect[1] = w1; rect[2] = h0; rect[3] = h1;
  return st;
}

int esc_tile_band(const esc_camera *cam, int32_t W, int32_t H, int32_t tile_x, int32_t row,
                  const float normal[3], double kp) {
  if (!cam || !normal || W < 2 || H < 2) {
    set_error("esc_tile_band: bad argument");
    return ESC_ERR_INVALID;
  }
  esc::RenderParams p;
  camera_params(cam, W, H, p);
  const esc::CamD c = esc::cam_frame(p);
  if (!c.ok) return 1;
  double fA = 0, fH = 0, fV = 0;
  for (int j = 0; j < 3; ++j) {
    fA += ((double)p.llc[j] - c.o[j]) * (double)normal[j];
    fH += (double)p.horizontal[j] * (double)normal[j];
    fV += (double)p.vertical[j] * (double)normal[j];
  }
  int tx0 = 0, tx1 = -1; // what k_bin_tri_escape does for this row
  if (!esc::band_row_tiles(p, c, row, (W + 31) / 32, fA, fH, fV, kp, tx0, tx1)) return 1;
  if (tile_x < tx0 || tile_x > tx1) return 0;
  double st[4], pmax;
  esc::tile_st_rect(p, c, tile_x, row, st, pmax);
  return esc::tile_band_hit(st, pmax, fA, fH, fV, kp) ? 1 : 0;
}

int esc_group_order(const float *xyz, int32_t count, int32_t run, int32_t big, int32_t huge,
                    int32_t *order) {
  if (!xyz || !order || count <= 0 || run <= 0 || big < run || huge < big || big % run || huge % big) {
    set_error("esc_group_order: bad argument");
    return ESC_ERR_INVALID;
  }
  std::vector<float> pts(xyz, xyz + 3 * (size_t)count);
  std::vector<int32_t> o;
  esc::group_order_points(pts, run, big, huge, o);
  std::memcpy(order, o.data(), sizeof(int32_t) * (size_t)count);
  return ESC_OK;
}

int esc_queue_schedule(int32_t n_triangles, int32_t n_spheres, int32_t *segments,
                       int32_t capacity) {
  if (n_triangles < 0 || n_spheres < 0 || capacity < 0 || (capacity && !segments)) {
    set_error("esc_queue_schedule: bad argument");
    return ESC_ERR_INVALID;
  }
  std::vector<int> segs;
  queue_segments(n_triangles, n_spheres, segs);
  const int n = (int)segs.size() / 4;
  if (n > capacity) {
    set_error("esc_queue_schedule: capacity too small");
    return ESC_ERR_INVALID;
  }
  std::copy(segs.begin(), segs.end(), segments);
  return n;
}

int esc_last_kernel_ms(esc_context *ctx, float ms[2]) {
  if (!ctx || !ms) {
    set_error("esc_last_kernel_ms: bad argument");
    return ESC_ERR_INVALID;
  }
  if (!ctx->ev_valid) {
    set_error("esc_last_kernel_ms: the last frame was not rendered with ESC_RENDER_TIME_KERNELS");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipEventSynchronize(ctx->ev[2]));
  HIP_TRY(hipEventElapsedTime(&ms[0], ctx->ev[0], ctx->ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms[1], ctx->ev[1], ctx->ev[2]));
  return ESC_OK;
}

int esc_last_frame_kernel(esc_context *ctx) {
  if (!ctx) {
    set_error("esc_last_frame_kernel: bad argument");
    return ESC_ERR_INVALID;
  }
  return ctx->last_frame_kernel;
}

int esc_frame_tripwire(esc_context *ctx) {
  if (!ctx) {
    set_error("esc_frame_tripwire: bad argument");
    return ESC_ERR_INVALID;
  }
  if (!ctx->ll.pk_total) return 0; // no light lists yet: no frame without fallback can have run
  HIP_TRY(hipSetDevice(ctx->device));
  int32_t w = 0;
  HIP_TRY(hipMemcpyAsync(&w, ctx->ll.pk_total + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->ll.pk_total + 2, 0, 4, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return w != 0 ? 1 : 0;
}

int esc_check_inv_det_exact(esc_context *ctx, uint32_t first_bits, uint64_t n, uint64_t *mismatches,
                            uint32_t *first_mismatch) {
  if (!ctx || !mismatches || !first_mismatch || n > (1ull << 32)) {
    set_error("esc_check_inv_det_exact: bad argument");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  unsigned long long *d_out = nullptr, h_out[2] = {0ull, ~0ull};
  int rc = ctx->call.alloc(d_out, 2);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d_out, h_out, sizeof(h_out), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = (hipError_t)esc_launch_check_inv_det(first_bits, n, d_out, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  rc = ctx->call.release(d_out);
  if (e != hipSuccess) {
    set_error(std::string("esc_check_inv_det_exact: ") + hipGetErrorString(e));
    return ESC_ERR_HIP;
  }
  if (rc) return rc;
  *mismatches = h_out[0];
  *first_mismatch = h_out[0] ? (uint32_t)h_out[1] : 0u;
  return ESC_OK;
}

int esc_scene_shadow_origins_inside(const esc_scene *scene, const float origin[3]) {
  if (!scene || !origin) {
    set_error("esc_scene_shadow_origins_inside: bad argument");
    return ESC_ERR_INVALID;
  }
  Staged s;
  int rc = stage_scene(*scene, s);
  if (rc) return rc;
  esc::SceneTables t;
  esc::build_scene_tables(s, t);
  return esc::shadow_origins_inside(origin, t.scene_lo, t.scene_hi, s.tri.data(), s.tri.size(),
                                    (int)s.lights.size())
             ? 1
             : 0;
}

// ---- batched ray queries (rt_query.hip) ---------------------------------------------------
// the per-scene tables every sweep of rt_query_sweep.h reads
static void query_tables(const esc_context *ctx, esc::QueryParams &p) {
  p.n_tri = ctx->n_tri;
  p.n_sph = ctx->n_sph;
  p.tri = ctx->d_tri;
  p.sph = ctx->d_sph;
  p.sph2_f = ctx->d_sph2_f;
  p.tri2_f = ctx->d_tri2_f;
  p.tri2_pf = ctx->d_tri2_pf;
  p.sg = ctx->sg;
  p.tg = ctx->tg;
  std::memcpy(p.g, ctx->shadow_center, sizeof(p.g));
  p.rho_max = ctx->shadow_rho_max;
}

static int query_launch(esc_context *ctx, const char *fn, bool occ, int64_t n, const float *d_origins,
                 const float *d_dirs, const float *d_tmax, float *d_t, int32_t *d_geom,
                 int32_t *d_prim, float *d_uv, uint8_t *d_occ, uint32_t flags) {
  if (!ctx) {
    set_error(std::string(fn) + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if (!ctx->have_scene) {
    set_error(std::string(fn) + ": no scene uploaded (esc_upload_scene / esc_upload_flat)");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error(std::string(fn) + ": n < 0");
    return ESC_ERR_INVALID;
  }
  if (flags & ~(uint32_t)ESC_RENDER_EXACT_ONLY) {
    set_error(std::string(fn) + ": flags takes 0 or ESC_RENDER_EXACT_ONLY only");
    return ESC_ERR_INVALID;
  }
  if (n > 0 && (!d_origins || !d_dirs || (occ ? !d_occ : (!d_t || !d_geom || !d_prim)))) {
    set_error(std::string(fn) + (occ ? ": d_origins, d_dirs and d_occluded are required"
                                     : ": d_origins, d_dirs, d_t, d_geom and d_prim are required"));
    return ESC_ERR_INVALID;
  }
  const uintptr_t bad = ((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_tmax |
                         (uintptr_t)d_t | (uintptr_t)d_geom | (uintptr_t)d_prim | (uintptr_t)d_uv) & 3u;
  if (bad) {
    set_error(std::string(fn) + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error(std::string(fn) + ": n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->d_qstats && ctx->call.alloc(ctx->d_qstats, 4)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_qstats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  if (n == 0) return ESC_OK;
  esc::QueryParams p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.orig = d_origins;
  p.dir = d_dirs;
  p.tmax = d_tmax;
  p.t = d_t;
  p.geom = d_geom;
  p.prim = d_prim;
  p.uv = d_uv;
  p.occ = d_occ;
  query_tables(ctx, p);
  p.exact_only = (flags & ESC_RENDER_EXACT_ONLY) ? 1 : 0;
  p.stats = ctx->d_qstats;
  const int e = esc_launch_query(&p, occ ? 1 : 0, ctx->stream);
  if (e) {
    set_error(std::string(fn) + ": k_query launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_intersect_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                       const float *d_tmax, float *d_t, int32_t *d_geom, int32_t *d_prim,
                       float *d_uv, uint32_t flags) {
  return query_launch(ctx, "esc_intersect_rays", false, n, d_origins, d_dirs, d_tmax, d_t, d_geom, d_prim,
                      d_uv, nullptr, flags);
}

int esc_occluded_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      const float *d_tmax, uint8_t *d_occluded, uint32_t flags) {
  return query_launch(ctx, "esc_occluded_rays", true, n, d_origins, d_dirs, d_tmax, nullptr, nullptr,
                      nullptr, nullptr, d_occluded, flags);
}

int esc_last_query_stats(esc_context *ctx, esc_query_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_query_stats: ctx is null" : "esc_last_query_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[4] = {0, 0, 0, 0};
  if (ctx->d_qstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_qstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->rays = h[0];
  out->exact_rays = h[1];
  out->exact_tests = h[2];
  return ESC_OK;
}

// ---- shading of caller-supplied rays, camera rays, supersampling (rt_shade_rays.hip) ---------------
// scratch of esc_render_supersampled: origins, directions and colours of one band (36 B per ray)
constexpr size_t kSsScratchBytes = size_t(256) << 20;
constexpr int kShadeStats = 5;

static int shade_options_ok(const esc_context *ctx, const char *fn, const esc_render_options *opts) {
  if (opts->flags & ~(int32_t)ESC_RENDER_EXACT_ONLY) {
    set_error(std::string(fn) + ": flags takes 0 or ESC_RENDER_EXACT_ONLY only");
    return ESC_ERR_INVALID;
  }
  if (opts->stage != ESC_STAGE_AUTO) {
    set_error(std::string(fn) + ": stage must be ESC_STAGE_AUTO");
    return ESC_ERR_INVALID;
  }
  if (opts->face_mode != ESC_FACE_FIXED && opts->face_mode != ESC_FACE_HASH) {
    set_error(std::string(fn) + ": face_mode must be ESC_FACE_FIXED or ESC_FACE_HASH");
    return ESC_ERR_INVALID;
  }
  if (opts->face_mode == ESC_FACE_FIXED &&
      (opts->fixed_face < 0 || (ctx->n_lights > 0 && opts->fixed_face >= ctx->min_light_faces))) {
    // main.cpp:743-748 draws faceID in [0, light.face_index.size())
    set_error(std::string(fn) + ": fixed_face must be in [0, face count of the smallest light)");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

static int shade_stats_reset(esc_context *ctx) {
  if (!ctx->d_sstats && ctx->call.alloc(ctx->d_sstats, kShadeStats)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_sstats, 0, kShadeStats * sizeof(unsigned long long), ctx->stream));
  return ESC_OK;
}

// the parameter block of k_shade_rays / k_trace for n rays of an already validated call
static void shade_params(esc_context *ctx, esc::ShadeParams &p, int64_t n, const float *d_origins,
                         const float *d_dirs, uint32_t pixel_base, const esc_render_options *opts, uint64_t seed,
                         float *d_rgb, uint8_t *d_rgb8) {
  std::memset(&p, 0, sizeof(p));
  p.q.n = n;
  p.q.orig = d_origins;
  p.q.dir = d_dirs;
  query_tables(ctx, p.q);
  p.q.exact_only = (opts->flags & ESC_RENDER_EXACT_ONLY) ? 1 : 0;
  p.rgb = d_rgb;
  p.rgb8 = d_rgb8;
  p.tri_n = ctx->d_tri_n;
  p.mat = ctx->d_mat;
  p.sph_mat = ctx->d_sph_mat;
  p.lights = ctx->d_lights;
  p.light_points = ctx->d_light_points;
  p.n_lights = ctx->n_lights;
  p.shadows = opts->shadows ? 1 : 0;
  p.face_mode = opts->face_mode;
  p.fixed_face = opts->fixed_face;
  p.seed = seed;
  p.pixel_base = pixel_base;
}

// k_shade_rays on n rays; the caller has validated everything and reset the stats
static int shade_launch(esc_context *ctx, const char *fn, int64_t n, const float *d_origins, const float *d_dirs,
                        uint32_t pixel_base, const esc_render_options *opts, uint64_t seed, float *d_rgb,
                        uint8_t *d_rgb8, float *d_t, int32_t *d_geom, int32_t *d_prim) {
  if (n == 0) return ESC_OK;
  esc::ShadeParams p;
  shade_params(ctx, p, n, d_origins, d_dirs, pixel_base, opts, seed, d_rgb, d_rgb8);
  p.t = d_t;
  p.geom = d_geom;
  p.prim = d_prim;
  p.stats = ctx->d_sstats;
  const int e = esc_launch_shade_rays(&p, ctx->stream);
  if (e) {
    set_error(std::string(fn) + ": k_shade_rays launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

static int camera_launch(esc_context *ctx, const char *fn, const esc_camera *cam, int32_t W, int32_t H,
                         int64_t pix0, int64_t n, const float *d_offsets, float dx, float dy, float *d_origins,
                         float *d_dirs) {
  if (n == 0) return ESC_OK;
  esc::CameraRayParams p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.origin, cam->origin, 12);
  std::memcpy(p.llc, cam->lower_left_corner, 12);
  std::memcpy(p.horizontal, cam->horizontal, 12);
  std::memcpy(p.vertical, cam->vertical, 12);
  p.W = W;
  p.H = H;
  p.pix0 = pix0;
  p.n = n;
  p.offsets = d_offsets;
  p.dx = dx;
  p.dy = dy;
  p.orig = d_origins;
  p.dir = d_dirs;
  const int e = esc_launch_camera_rays(&p, ctx->stream);
  if (e) {
    set_error(std::string(fn) + ": k_camera_rays launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_camera_rays(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t row_begin,
                    int32_t row_end, const float *d_offsets, float *d_origins, float *d_dirs) {
  const char *fn = "esc_camera_rays";
  if (!ctx || !cam) {
    set_error(!ctx ? "esc_camera_rays: ctx is null" : "esc_camera_rays: cam is null");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2 || row_begin < 0 || row_end > H || row_begin > row_end) {
    set_error("esc_camera_rays: need W,H >= 2 and 0 <= row_begin <= row_end <= H");
    return ESC_ERR_INVALID;
  }
  const int64_t n = (int64_t)(row_end - row_begin) * W;
  if (n > 0 && (!d_origins || !d_dirs)) {
    set_error("esc_camera_rays: d_origins and d_dirs are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_offsets | (uintptr_t)d_origins | (uintptr_t)d_dirs) & 3u) {
    set_error("esc_camera_rays: device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_camera_rays: too many rays for one launch");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  return camera_launch(ctx, fn, cam, W, H, (int64_t)row_begin * W, n, d_offsets, 0.f, 0.f, d_origins, d_dirs);
}

int esc_shade_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t pixel_base,
                   const esc_render_options *opts, float *d_rgb, uint8_t *d_rgb8, float *d_t, int32_t *d_geom,
                   int32_t *d_prim) {
  const char *fn = "esc_shade_rays";
  if (!ctx || !opts) {
    set_error(!ctx ? "esc_shade_rays: ctx is null" : "esc_shade_rays: opts is null");
    return ESC_ERR_INVALID;
  }
  if (!ctx->have_scene) {
    set_error("esc_shade_rays: no scene uploaded (esc_upload_scene / esc_upload_flat)");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error("esc_shade_rays: n < 0");
    return ESC_ERR_INVALID;
  }
  int rc = shade_options_ok(ctx, fn, opts);
  if (rc) return rc;
  if (n > 0 && (!d_origins || !d_dirs || !d_rgb)) {
    set_error("esc_shade_rays: d_origins, d_dirs and d_rgb are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_rgb | (uintptr_t)d_t | (uintptr_t)d_geom |
       (uintptr_t)d_prim) & 3u) {
    set_error("esc_shade_rays: device pointers must be 4-byte aligned (d_rgb8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_shade_rays: n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if ((rc = shade_stats_reset(ctx))) return rc;
  return shade_launch(ctx, fn, n, d_origins, d_dirs, pixel_base, opts, opts->seed, d_rgb, d_rgb8, d_t, d_geom,
                      d_prim);
}

int esc_last_shade_stats(esc_context *ctx, esc_shade_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_shade_stats: ctx is null" : "esc_last_shade_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[kShadeStats] = {0, 0, 0, 0, 0};
  if (ctx->d_sstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_sstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->rays = h[0];
  out->hit_rays = h[1];
  out->shadow_rays = h[2];
  out->exact_rays = h[3];
  out->exact_tests = h[4];
  return ESC_OK;
}

// argument checks of the supersampled / traced frames; nn receives n of spp = n*n
static int frame_args_ok(esc_context *ctx, const char *fn_, const esc_camera *cam, int32_t W, int32_t H,
                         int32_t spp, const esc_render_options *opts, float *d_image, int &nn) {
  const std::string fn(fn_);
  if (!ctx || !cam || !opts || !d_image) {
    set_error(!ctx ? fn + ": ctx is null" : fn + ": bad argument");
    return ESC_ERR_INVALID;
  }
  nn = 0;
  for (int k = 1; k <= 8; ++k)
    if (k * k == spp) nn = k;
  if (!nn) {
    set_error(fn + ": spp must be n*n with n in 1..8");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error(fn + ": need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  if ((int64_t)W * H > 0x7fffffffLL) {
    set_error(fn + ": W*H exceeds the reference's int pixel index (main.cpp:784)");
    return ESC_ERR_INVALID;
  }
  if (!ctx->have_scene) {
    set_error(fn + ": no scene uploaded");
    return ESC_ERR_INVALID;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->lower_left_corner[k]) ||
        !std::isfinite(cam->horizontal[k]) || !std::isfinite(cam->vertical[k])) {
      set_error(fn + ": camera is not finite");
      return ESC_ERR_INVALID;
    }
  const int rc = shade_options_ok(ctx, fn_, opts);
  if (rc) return rc;
  if (((uintptr_t)d_image) & 3u) {
    set_error(fn + ": d_image must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

int esc_render_supersampled(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                            const esc_render_options *opts, float *d_image, uint8_t *d_u8) {
  const char *fn = "esc_render_supersampled";
  int nn = 0;
  int rc = frame_args_ok(ctx, fn, cam, W, H, spp, opts, d_image, nn);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // bands of whole rows (of pixels when one row does not fit) within the scratch budget
  const int64_t total = (int64_t)W * H;
  int64_t band = std::min<int64_t>(total, (int64_t)(kSsScratchBytes / (9 * sizeof(float))));
  if (band >= W) band -= band % W;
  if ((rc = ctx->call.grow(ctx->d_ss, ctx->ss_floats, (size_t)band * 9))) return rc;
  float *d_o = ctx->d_ss, *d_d = ctx->d_ss + 3 * (size_t)band, *d_rgb = ctx->d_ss + 6 * (size_t)band;
  if ((rc = shade_stats_reset(ctx))) return rc;
  for (int64_t p0 = 0; p0 < total; p0 += band) {
    const int64_t n = std::min(band, total - p0);
    float *img = d_image + 3 * p0;
    for (int k = 0; k < spp; ++k) {
      // sample k = j*n + i at (i + 1/2)/n - 1/2, (j + 1/2)/n - 1/2 pixels (fp32)
      const float dx = ((float)(k % nn) + 0.5f) / (float)nn - 0.5f;
      const float dy = ((float)(k / nn) + 0.5f) / (float)nn - 0.5f;
      if ((rc = camera_launch(ctx, fn, cam, W, H, p0, n, nullptr, dx, dy, d_o, d_d))) return rc;
      if ((rc = shade_launch(ctx, fn, n, d_o, d_d, (uint32_t)p0, opts, opts->seed + (uint64_t)k, d_rgb, nullptr,
                             nullptr, nullptr, nullptr)))
        return rc;
      const int e = esc_launch_ss_accumulate(img, d_rgb, 3 * n, k == 0 ? 1 : 0, ctx->stream);
      if (e) {
        set_error(std::string(fn) + ": k_ss_accumulate launch: " + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
    }
    const int e = esc_launch_ss_finish(img, d_u8 ? d_u8 + 3 * p0 : nullptr, 3 * n, (float)spp, ctx->stream);
    if (e) {
      set_error(std::string(fn) + ": k_ss_finish launch: " + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  return ESC_OK;
}


// ---- adaptive supersampling (rt_adaptive.hip) ------------------------------------------------------
constexpr int kAdaptiveWords = esc::kAdaptiveStats + 1; // esc_adaptive_stats' counters, then the list's counter

int esc_render_adaptive(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                        const esc_render_options *opts, const esc_adaptive_options *aopts, float *d_image,
                        uint8_t *d_u8, uint8_t *d_mask) {
  const char *fn = "esc_render_adaptive";
  if (ctx && !aopts) {
    set_error(std::string(fn) + ": adaptive options are null");
    return ESC_ERR_INVALID;
  }
  int nn = 0;
  int rc = frame_args_ok(ctx, fn, cam, W, H, aopts ? aopts->spp : 1, opts, d_image, nn);
  if (rc) return rc;
  if (!(aopts->threshold >= 0.f) || !std::isfinite(aopts->threshold)) {
    set_error(std::string(fn) + ": threshold must be a finite number >= 0");
    return ESC_ERR_INVALID;
  }
  if (aopts->reserved != 0) {
    set_error(std::string(fn) + ": reserved must be 0");
    return ESC_ERR_INVALID;
  }
  if (aopts->band_rows < 0) {
    set_error(std::string(fn) + ": band_rows must be 0 (automatic) or a positive row count");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  // bands of whole rows (of pixels when one row does not fit) whose list stays within the scratch budget
  const int64_t total = (int64_t)W * H;
  int64_t band = std::min<int64_t>(total, (int64_t)(kSsScratchBytes / sizeof(uint32_t)));
  if (band >= W) band -= band % W;
  if (aopts->band_rows > 0) band = std::min<int64_t>(total, (int64_t)aopts->band_rows * W);
  const size_t list_bytes = ((size_t)band * sizeof(uint32_t) + 255) & ~(size_t)255;
  const size_t need = list_bytes + (d_mask ? 0 : (size_t)total);
  if ((rc = ctx->call.grow(ctx->d_ad, ctx->ad_bytes, need))) return rc;
  if (!ctx->d_astats && (rc = ctx->call.alloc(ctx->d_astats, kAdaptiveWords))) return rc;
  uint32_t *d_list = (uint32_t *)ctx->d_ad;
  uint8_t *mask = d_mask ? d_mask : ctx->d_ad + list_bytes;
  uint32_t *d_count = (uint32_t *)(ctx->d_astats + esc::kAdaptiveStats);

  // 1. the base frame B, on the frame path
  if ((rc = esc_render_rows(ctx, cam, W, H, 0, H, opts, d_image, d_u8))) return rc;
  HIP_TRY(hipMemsetAsync(ctx->d_astats, 0, kAdaptiveWords * sizeof(unsigned long long), ctx->stream));
  ctx->ad_pixels = (uint64_t)total;
  ctx->ad_spp = aopts->spp;
  // 2. the mask of the whole frame, before any pixel is refined in place
  esc::AdaptiveMaskParams mp;
  std::memset(&mp, 0, sizeof(mp));
  mp.image = d_image;
  mp.mask = mask;
  mp.W = W;
  mp.H = H;
  mp.threshold = aopts->threshold;
  int e = esc_launch_adaptive_mask(&mp, ctx->stream);
  if (e) {
    set_error(std::string(fn) + ": k_adaptive_mask launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  // 3. per band: list the masked pixels, refine the listed ones
  esc::AdaptiveRefineParams rp;
  std::memset(&rp, 0, sizeof(rp));
  shade_params(ctx, rp.s, 0, nullptr, nullptr, 0, opts, opts->seed, d_image, d_u8);
  rp.s.stats = ctx->d_astats;
  std::memcpy(rp.origin, cam->origin, 12);
  std::memcpy(rp.llc, cam->lower_left_corner, 12);
  std::memcpy(rp.horizontal, cam->horizontal, 12);
  std::memcpy(rp.vertical, cam->vertical, 12);
  rp.W = W;
  rp.H = H;
  rp.spp = aopts->spp;
  rp.nn = nn;
  rp.list = d_list;
  rp.count = d_count;
  for (int64_t p0 = 0; p0 < total; p0 += band) {
    const int64_t n = std::min(band, total - p0);
    if (p0 > 0) HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), ctx->stream));
    esc::AdaptiveListParams lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.mask = mask;
    lp.list = d_list;
    lp.count = d_count;
    lp.pix0 = p0;
    lp.n = n;
    if ((e = esc_launch_adaptive_list(&lp, ctx->stream))) {
      set_error(std::string(fn) + ": k_adaptive_list launch: " + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
    rp.s.q.n = n;
    if ((e = esc_launch_adaptive_refine(&rp, ctx->stream))) {
      set_error(std::string(fn) + ": k_adaptive_refine launch: " + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  return ESC_OK;
}

int esc_last_adaptive_stats(esc_context *ctx, esc_adaptive_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_adaptive_stats: ctx is null" : "esc_last_adaptive_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kAdaptiveStats] = {0, 0, 0, 0, 0};
  if (ctx->d_astats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_astats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->pixels = ctx->ad_pixels;
  out->refined_pixels = h[0];
  out->samples = h[0] * (uint64_t)ctx->ad_spp;
  out->hit_rays = h[1];
  out->shadow_rays = h[2];
  out->exact_rays = h[3];
  out->exact_tests = h[4];
  return ESC_OK;
}

// ---- mirror reflections (rt_trace.hip) -------------------------------------------------------------
constexpr int kTraceStatWords = esc::kTraceStats + esc::kTransmitStats; // esc_trace_stats, esc_transmit_stats
constexpr int kTraceCounters = esc::kTraceMaxDepth + 2; // uint32 queue counters, after the stats
constexpr size_t kTraceQueueBytes = 2 * esc::kTraceQueuePlanes * sizeof(float); // both queues, per ray

static int trace_args_ok(const char *fn, int32_t max_depth, float bias) {
  if (max_depth < 0 || max_depth > ESC_TRACE_MAX_DEPTH) {
    set_error(std::string(fn) + ": max_depth must be in 0..16");
    return ESC_ERR_INVALID;
  }
  if (!(bias >= 0.f) || !std::isfinite(bias)) {
    set_error(std::string(fn) + ": bias must be finite and >= 0");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

static int trace_stats_reset(esc_context *ctx) {
  const size_t words = kTraceStatWords + (kTraceCounters * sizeof(uint32_t) + 7) / 8; // the stats, then the counters
  if (!ctx->d_tstats && ctx->call.alloc(ctx->d_tstats, words)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_tstats, 0, kTraceStatWords * sizeof(unsigned long long), ctx->stream));
  return ESC_OK;
}

// grow-only scratch of the bounce loop.  No recorded frame reads it, so no epoch is involved.
static int trace_scratch(esc_context *ctx, size_t bytes) {
  return ctx->call.grow(ctx->d_tr, ctx->tr_floats, bytes / sizeof(float));
}

// the bounce loop on one batch of n rays: levels 0 .. max_depth, one launch each, nothing waited for.
// d_queues: 2 * kTraceQueuePlanes * n floats.  The caller has validated everything and reset the stats.
static int trace_launch(esc_context *ctx, const char *fn, int64_t n, const float *d_origins, const float *d_dirs,
                        uint32_t pixel_base, const esc_render_options *opts, uint64_t seed, int32_t max_depth,
                        float bias, int32_t transmission, float *d_rgb, uint8_t *d_rgb8, float *d_queues) {
  if (n == 0) return ESC_OK;
  uint32_t *cnt = reinterpret_cast<uint32_t *>(ctx->d_tstats + kTraceStatWords);
  HIP_TRY(hipMemsetAsync(cnt, 0, kTraceCounters * sizeof(uint32_t), ctx->stream));
  esc::TraceParams p;
  std::memset(&p, 0, sizeof(p));
  shade_params(ctx, p.s, n, d_origins, d_dirs, pixel_base, opts, seed, d_rgb, d_rgb8);
  p.s.stats = ctx->d_tstats;
  p.max_depth = max_depth;
  p.bias = bias;
  if (transmission != ESC_TRANSMIT_OFF && ctx->any_transmissive) { // else the mirror-only kernels
    p.transmit = ctx->d_transmit;
    p.transmit_mode = transmission;
  }
  p.env.texels = ctx->d_env; // null: the kernels without the lookup
  p.env.res = ctx->env_res;
  float *queue[2] = {d_queues, d_queues + (size_t)esc::kTraceQueuePlanes * (size_t)n};
  for (int k = 0; k <= max_depth; ++k) {
    p.level = k;
    p.s.seed = seed + 64ull * (uint64_t)k;
    p.q_in = queue[k & 1];
    p.q_out = queue[(k + 1) & 1];
    p.n_in = cnt + k; // counter k: the rays of level k, written by level k - 1
    p.n_out = cnt + k + 1;
    const int e = esc_launch_trace_level(&p, ctx->stream);
    if (e) {
      set_error(std::string(fn) + ": k_trace launch: " + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  return ESC_OK;
}

// the mode and the reserved word of esc_trace_options
static int transmit_args_ok(const char *fn, const esc_trace_options *topts) {
  if (topts->transmission < ESC_TRANSMIT_OFF || topts->transmission > ESC_TRANSMIT_FRESNEL) {
    set_error(std::string(fn) + ": transmission must be ESC_TRANSMIT_OFF, _REFRACT or _FRESNEL");
    return ESC_ERR_INVALID;
  }
  if (topts->reserved != 0) {
    set_error(std::string(fn) + ": reserved must be 0");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

static int trace_rays_impl(const char *fn_, esc_context *ctx, int64_t n, const float *d_origins,
                           const float *d_dirs, uint32_t pixel_base, const esc_render_options *opts,
                           int32_t max_depth, float bias, int32_t transmission, float *d_rgb, uint8_t *d_rgb8) {
  const std::string fn(fn_);
  if (!ctx->have_scene) {
    set_error(fn + ": no scene uploaded (esc_upload_scene / esc_upload_flat)");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error(fn + ": n < 0");
    return ESC_ERR_INVALID;
  }
  int rc = shade_options_ok(ctx, fn_, opts);
  if (rc) return rc;
  if ((rc = trace_args_ok(fn_, max_depth, bias))) return rc;
  if (n > 0 && (!d_origins || !d_dirs || !d_rgb)) {
    set_error(fn + ": d_origins, d_dirs and d_rgb are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_rgb) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned (d_rgb8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error(fn + ": n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if ((rc = trace_stats_reset(ctx))) return rc;
  // batches of rays whose two queues fit the scratch budget (none is needed at depth 0)
  const int64_t batch = max_depth == 0 ? n : std::min<int64_t>(n, (int64_t)(kSsScratchBytes / kTraceQueueBytes));
  if (max_depth > 0 && (rc = trace_scratch(ctx, (size_t)batch * kTraceQueueBytes))) return rc;
  for (int64_t r0 = 0; r0 < n; r0 += batch) {
    const int64_t m = std::min(batch, n - r0);
    if ((rc = trace_launch(ctx, fn_, m, d_origins + 3 * r0, d_dirs + 3 * r0, pixel_base + (uint32_t)r0, opts,
                           opts->seed, max_depth, bias, transmission, d_rgb + 3 * r0,
                           d_rgb8 ? d_rgb8 + 3 * r0 : nullptr, ctx->d_tr)))
      return rc;
  }
  return ESC_OK;
}

int esc_trace_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t pixel_base,
                   const esc_render_options *opts, int32_t max_depth, float bias, float *d_rgb, uint8_t *d_rgb8) {
  if (!ctx || !opts) {
    set_error(!ctx ? "esc_trace_rays: ctx is null" : "esc_trace_rays: opts is null");
    return ESC_ERR_INVALID;
  }
  return trace_rays_impl("esc_trace_rays", ctx, n, d_origins, d_dirs, pixel_base, opts, max_depth, bias,
                         ESC_TRANSMIT_OFF, d_rgb, d_rgb8);
}

int esc_trace_rays_ex(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      uint32_t pixel_base, const esc_render_options *opts, const esc_trace_options *topts,
                      float *d_rgb, uint8_t *d_rgb8) {
  const char *fn = "esc_trace_rays_ex";
  if (!ctx || !opts || !topts) {
    set_error(!ctx ? "esc_trace_rays_ex: ctx is null"
                   : !opts ? "esc_trace_rays_ex: opts is null" : "esc_trace_rays_ex: trace options are null");
    return ESC_ERR_INVALID;
  }
  const int rc = transmit_args_ok(fn, topts);
  if (rc) return rc;
  return trace_rays_impl(fn, ctx, n, d_origins, d_dirs, pixel_base, opts, topts->max_depth, topts->bias,
                         topts->transmission, d_rgb, d_rgb8);
}

int esc_last_transmit_stats(esc_context *ctx, esc_transmit_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_transmit_stats: ctx is null" : "esc_last_transmit_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kTransmitStats] = {0};
  if (ctx->d_tstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_tstats + esc::kTraceStats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->refracted = h[0];
  out->fresnel_reflected = h[1];
  out->total_internal = h[2];
  return ESC_OK;
}

int esc_last_trace_stats(esc_context *ctx, esc_trace_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_trace_stats: ctx is null" : "esc_last_trace_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kTraceStats] = {0};
  if (ctx->d_tstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_tstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->rays = 0; // the kernel keeps the rays per level only (rt_trace.hip)
  out->hit_rays = h[1];
  out->shadow_rays = h[2];
  out->exact_rays = h[3];
  out->exact_tests = h[4];
  for (int k = 0; k <= ESC_TRACE_MAX_DEPTH; ++k) {
    out->depth_rays[k] = h[5 + k];
    out->rays += h[5 + k];
  }
  return ESC_OK;
}

// A ray maker of the traced frame: writes the n rays of sample k of pixels [p0, p0 + n) with the sub-pixel
// offset (dx, dy).  arg: the maker's own (pinhole_rays: unused; lens_frame_rays: the esc_lens_options)
typedef int (*RayMaker)(esc_context *ctx, const char *fn, const esc_camera *cam, int32_t W, int32_t H,
                        const void *arg, int k, int64_t p0, int64_t n, float dx, float dy, float *d_o, float *d_d);

// the pinhole rays of a band's sample: esc_render_supersampled's (k is the lens sample, which a pinhole has not)
static int pinhole_rays(esc_context *ctx, const char *fn, const esc_camera *cam, int32_t W, int32_t H, const void *,
                        int, int64_t p0, int64_t n, float dx, float dy, float *d_o, float *d_d) {
  return camera_launch(ctx, fn, cam, W, H, p0, n, nullptr, dx, dy, d_o, d_d);
}

// The traced frame's loop over bands x samples: make_rays -> trace_launch -> k_ss_accumulate -> k_ss_finish
static int render_traced_impl(const char *fn, esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                              int32_t spp, int32_t max_depth, float bias, int32_t transmission,
                              const esc_render_options *opts, float *d_image, uint8_t *d_u8,
                              RayMaker make_rays, const void *maker_arg) {
  int nn = 0;
  int rc = frame_args_ok(ctx, fn, cam, W, H, spp, opts, d_image, nn);
  if (rc) return rc;
  if ((rc = trace_args_ok(fn, max_depth, bias))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // bands of whole rows (of pixels when one row does not fit): origins, directions, colours and, past
  // depth 0, both queues of a band within the scratch budget
  const size_t per_ray = 9 * sizeof(float) + (max_depth > 0 ? kTraceQueueBytes : 0);
  const int64_t total = (int64_t)W * H;
  int64_t band = std::min<int64_t>(total, (int64_t)(kSsScratchBytes / per_ray));
  if (band >= W) band -= band % W;
  if ((rc = trace_scratch(ctx, (size_t)band * per_ray))) return rc;
  float *d_o = ctx->d_tr, *d_d = d_o + 3 * (size_t)band, *d_rgb = d_o + 6 * (size_t)band;
  float *d_queues = d_o + 9 * (size_t)band;
  if ((rc = trace_stats_reset(ctx))) return rc;
  for (int64_t p0 = 0; p0 < total; p0 += band) {
    const int64_t n = std::min(band, total - p0);
    float *img = d_image + 3 * p0;
    for (int k = 0; k < spp; ++k) {
      // esc_render_supersampled's sample k
      const float dx = ((float)(k % nn) + 0.5f) / (float)nn - 0.5f;
      const float dy = ((float)(k / nn) + 0.5f) / (float)nn - 0.5f;
      if ((rc = make_rays(ctx, fn, cam, W, H, maker_arg, k, p0, n, dx, dy, d_o, d_d))) return rc;
      if ((rc = trace_launch(ctx, fn, n, d_o, d_d, (uint32_t)p0, opts, opts->seed + (uint64_t)k, max_depth, bias,
                             transmission, d_rgb, nullptr, d_queues)))
        return rc;
      const int e = esc_launch_ss_accumulate(img, d_rgb, 3 * n, k == 0 ? 1 : 0, ctx->stream);
      if (e) {
        set_error(std::string(fn) + ": k_ss_accumulate launch: " + hipGetErrorString((hipError_t)e));
        return ESC_ERR_HIP;
      }
    }
    const int e = esc_launch_ss_finish(img, d_u8 ? d_u8 + 3 * p0 : nullptr, 3 * n, (float)spp, ctx->stream);
    if (e) {
      set_error(std::string(fn) + ": k_ss_finish launch: " + hipGetErrorString((hipError_t)e));
      return ESC_ERR_HIP;
    }
  }
  return ESC_OK;
}

int esc_render_traced(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                      int32_t max_depth, float bias, const esc_render_options *opts, float *d_image,
                      uint8_t *d_u8) {
  return render_traced_impl("esc_render_traced", ctx, cam, W, H, spp, max_depth, bias, ESC_TRANSMIT_OFF, opts,
                            d_image, d_u8, pinhole_rays, nullptr);
}

int esc_render_traced_ex(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                         const esc_render_options *opts, const esc_trace_options *topts, float *d_image,
                         uint8_t *d_u8) {
  const char *fn = "esc_render_traced_ex";
  if (!ctx || !topts) {
    set_error(!ctx ? "esc_render_traced_ex: ctx is null" : "esc_render_traced_ex: trace options are null");
    return ESC_ERR_INVALID;
  }
  const int rc = transmit_args_ok(fn, topts);
  if (rc) return rc;
  return render_traced_impl(fn, ctx, cam, W, H, spp, topts->max_depth, topts->bias, topts->transmission, opts,
                            d_image, d_u8, pinhole_rays, nullptr);
}

// ---- thin-lens camera (rt_lens.h, rt_lens.hip) -----------------------------------------------------
int esc_lens_disk_table(int32_t sets, int32_t samples, uint64_t seed, float *out) {
  const char *fn = "esc_lens_disk_table";
  if (sets < 1 || sets > esc::kLensMaxDim || samples < 1 || samples > esc::kLensMaxDim) {
    set_error(std::string(fn) + ": sets and samples must be in 1..64");
    return ESC_ERR_INVALID;
  }
  if (!out) {
    set_error(std::string(fn) + ": out is null");
    return ESC_ERR_INVALID;
  }
  // splitmix64 from (seed, sets, samples), tagged so that the stream is not the ambient table's
  uint64_t st = seed ^ ((uint64_t)sets << 48) ^ ((uint64_t)samples << 40) ^ 0x4C454E53ull;
  auto next = [&st]() {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return ((double)(z >> 11) + 0.5) * 0x1p-53;
  };
  int grid = 0; // n when samples == n*n: one jittered point per cell
  for (int n = 1; n <= 8; ++n)
    if (n * n == samples) grid = n;
  const double quarter_pi = 0.78539816339744830961566084581988, half_pi = 1.5707963267948966192313216916398;
  for (int32_t s = 0; s < sets; ++s) {
    float *row = out + 2 * (size_t)s * samples;
    for (int32_t c = 0; c < samples; ++c) {
      const double u1 = next(), u2 = next();
      const double x = grid ? ((double)(c % grid) + u1) / (double)grid : ((double)c + u1) / (double)samples;
      const double y = grid ? ((double)(c / grid) + u2) / (double)grid : u2;
      // the concentric map of the square [-1, 1]^2 onto the unit disk
      const double a = 2.0 * x - 1.0, b = 2.0 * y - 1.0;
      double r = 0.0, phi = 0.0;
      if (a != 0.0 || b != 0.0) {
        if (std::fabs(a) > std::fabs(b)) {
          r = a;
          phi = quarter_pi * (b / a);
        } else {
          r = b;
          phi = half_pi - quarter_pi * (a / b);
        }
      }
      float fx = (float)(r * std::cos(phi)), fy = (float)(r * std::sin(phi));
      while ((double)fx * fx + (double)fy * fy > 1.0) { // the casts may have rounded a rim point outwards
        fx *= 1.f - 0x1p-24f;
        fy *= 1.f - 0x1p-24f;
      }
      row[2 * c] = fx;
      row[2 * c + 1] = fy;
    }
    for (int32_t m = samples - 1; m >= 1; --m) { // Fisher-Yates: lens sample k is not sub-pixel cell k
      int32_t j = (int32_t)(next() * (double)(m + 1));
      if (j > m) j = m;
      std::swap(row[2 * m], row[2 * j]);
      std::swap(row[2 * m + 1], row[2 * j + 1]);
    }
  }
  return ESC_OK;
}

int esc_set_lens_table(esc_context *ctx, int32_t sets, int32_t samples, const float *host_table) {
  const char *fn = "esc_set_lens_table";
  if (!ctx) {
    set_error(std::string(fn) + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if ((sets == 0) != (host_table == nullptr)) {
    set_error(std::string(fn) + ": sets == 0 goes with host_table == NULL (no table), and only with it");
    return ESC_ERR_INVALID;
  }
  if (sets != 0 && (sets < 1 || sets > esc::kLensMaxDim || samples < 1 || samples > esc::kLensMaxDim)) {
    set_error(std::string(fn) + ": sets and samples must be in 1..64");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // a call in flight may still read the old table
  ctx->lens_sets = ctx->lens_samples = 0;
  const size_t floats = sets ? (size_t)sets * samples * 2 : 0;
  const int rc = ctx->call.alloc(ctx->d_lens, floats); // sets == 0: freed, stays null
  if (rc || sets == 0) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->d_lens, host_table, floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // host_table is the caller's again
  ctx->lens_sets = sets;
  ctx->lens_samples = samples;
  return ESC_OK;
}

int esc_get_lens_table_shape(esc_context *ctx, int32_t *sets, int32_t *samples) {
  if (!ctx || !sets || !samples) {
    set_error(!ctx ? "esc_get_lens_table_shape: ctx is null" : "esc_get_lens_table_shape: sets or samples is null");
    return ESC_ERR_INVALID;
  }
  *sets = ctx->lens_sets;
  *samples = ctx->lens_samples;
  return ESC_OK;
}

// the lens checks esc_lens_rays and esc_render_lens share, after ctx and lens are known not to be null.
// last: the highest lens sample the call reads (`what` names the argument it comes from)
static int lens_options_ok(const esc_context *ctx, const char *fn_, const esc_lens_options *lens, int32_t last,
                           const char *what) {
  const std::string fn(fn_);
  if (!(lens->aperture >= 0.f) || !std::isfinite(lens->aperture)) {
    set_error(fn + ": aperture must be finite and >= 0");
    return ESC_ERR_INVALID;
  }
  if (!(lens->focus_dist > 0.f) || !std::isfinite(lens->focus_dist)) {
    set_error(fn + ": focus_dist must be finite and > 0");
    return ESC_ERR_INVALID;
  }
  if (lens->reserved[0] != 0 || lens->reserved[1] != 0) {
    set_error(fn + ": reserved must be 0");
    return ESC_ERR_INVALID;
  }
  if (last < 0) {
    set_error(fn + ": " + what + " is negative");
    return ESC_ERR_INVALID;
  }
  if (lens->aperture == 0.f) return ESC_OK; // a pinhole reads no table
  if (!ctx->d_lens) {
    set_error(fn + ": no lens table (esc_set_lens_table) while aperture > 0");
    return ESC_ERR_INVALID;
  }
  if (last >= ctx->lens_samples) {
    set_error(fn + ": " + what + " is beyond the lens table's samples per set");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

// k_lens_rays on n rays of an already validated call
static int lens_launch(esc_context *ctx, const char *fn, const esc_camera *cam, int32_t W, int32_t H, int64_t pix0,
                       int64_t n, const float *d_offsets, float dx, float dy, const esc_lens_options *lens,
                       int32_t sample, float *d_origins, float *d_dirs) {
  if (n == 0) return ESC_OK;
  esc::LensRayParams p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.origin, cam->origin, 12);
  std::memcpy(p.llc, cam->lower_left_corner, 12);
  std::memcpy(p.horizontal, cam->horizontal, 12);
  std::memcpy(p.vertical, cam->vertical, 12);
  esc::lens_axis(cam->horizontal, p.U);
  esc::lens_axis(cam->vertical, p.V);
  p.aperture = lens->aperture;
  p.focus_dist = lens->focus_dist;
  p.W = W;
  p.H = H;
  p.pix0 = pix0;
  p.n = n;
  p.offsets = d_offsets;
  p.dx = dx;
  p.dy = dy;
  p.table = ctx->d_lens;
  p.sets = ctx->lens_sets;
  p.samples = ctx->lens_samples;
  p.sample = sample;
  p.seed = lens->seed;
  p.orig = d_origins;
  p.dir = d_dirs;
  const int e = esc_launch_lens_rays(&p, ctx->stream);
  if (e) {
    set_error(std::string(fn) + ": k_lens_rays launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_lens_rays(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t row_begin,
                  int32_t row_end, const float *d_offsets, const esc_lens_options *lens, int32_t sample,
                  float *d_origins, float *d_dirs) {
  const char *fn = "esc_lens_rays";
  if (!ctx || !cam || !lens) {
    set_error(!ctx ? "esc_lens_rays: ctx is null" : !cam ? "esc_lens_rays: cam is null"
                                                         : "esc_lens_rays: lens options are null");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2 || row_begin < 0 || row_end > H || row_begin > row_end) {
    set_error("esc_lens_rays: need W,H >= 2 and 0 <= row_begin <= row_end <= H");
    return ESC_ERR_INVALID;
  }
  const int rc = lens_options_ok(ctx, fn, lens, sample, "sample");
  if (rc) return rc;
  const int64_t n = (int64_t)(row_end - row_begin) * W;
  if (n > 0 && (!d_origins || !d_dirs)) {
    set_error("esc_lens_rays: d_origins and d_dirs are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_offsets | (uintptr_t)d_origins | (uintptr_t)d_dirs) & 3u) {
    set_error("esc_lens_rays: device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_lens_rays: too many rays for one launch");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  return lens_launch(ctx, fn, cam, W, H, (int64_t)row_begin * W, n, d_offsets, 0.f, 0.f, lens, sample, d_origins,
                     d_dirs);
}

// the lens rays of a band's sample: lens sample k (a RayMaker; arg: the call's esc_lens_options)
static int lens_frame_rays(esc_context *ctx, const char *fn, const esc_camera *cam, int32_t W, int32_t H,
                           const void *arg, int k, int64_t p0, int64_t n, float dx, float dy, float *d_o,
                           float *d_d) {
  return lens_launch(ctx, fn, cam, W, H, p0, n, nullptr, dx, dy, static_cast<const esc_lens_options *>(arg), k, d_o,
                     d_d);
}

int esc_render_lens(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, int32_t spp,
                    const esc_render_options *opts, const esc_trace_options *topts, const esc_lens_options *lens,
                    float *d_image, uint8_t *d_u8) {
  const char *fn = "esc_render_lens";
  if (!ctx || !topts || !lens) {
    set_error(!ctx ? "esc_render_lens: ctx is null"
                   : !topts ? "esc_render_lens: trace options are null" : "esc_render_lens: lens options are null");
    return ESC_ERR_INVALID;
  }
  int rc = transmit_args_ok(fn, topts);
  if (rc) return rc;
  if (spp < 1) {
    set_error(std::string(fn) + ": spp must be n*n with n in 1..8");
    return ESC_ERR_INVALID;
  }
  if ((rc = lens_options_ok(ctx, fn, lens, spp - 1, "spp"))) return rc;
  return render_traced_impl(fn, ctx, cam, W, H, spp, topts->max_depth, topts->bias, topts->transmission, opts,
                            d_image, d_u8, lens_frame_rays, lens);
}

// ---- environment cube map (rt_environ.h, rt_environ.hip) -------------------------------------------
// texels[face][j][i][3] -> one 16-byte record per texel, the layout the kernels read
static void env_repack(int32_t res, const float *texels, std::vector<esc::EnvTexel> &out) {
  const size_t n = (size_t)6 * (size_t)res * (size_t)res;
  out.resize(n);
  for (size_t k = 0; k < n; ++k) out[k] = esc::EnvTexel{texels[3 * k], texels[3 * k + 1], texels[3 * k + 2], 0.f};
}

int esc_set_environment(esc_context *ctx, int32_t res, const float *host_texels) {
  const char *fn = "esc_set_environment";
  if (!ctx) {
    set_error(std::string(fn) + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if (res < 0 || res > esc::kEnvMaxRes) {
    set_error(std::string(fn) + ": res must be in 0..1024");
    return ESC_ERR_INVALID;
  }
  if ((res == 0) != (host_texels == nullptr)) {
    set_error(std::string(fn) + ": res == 0 goes with host_texels == NULL (no environment), and only with it");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // a call in flight may still read the old cube
  ctx->env_res = 0;
  std::vector<esc::EnvTexel> packed;
  if (res) env_repack(res, host_texels, packed);
  const int rc = upload_vec(ctx->call, ctx->d_env, packed, ctx->stream); // res == 0: freed, stays null
  if (rc || res == 0) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // `packed` goes out of scope
  ctx->env_res = res;
  return ESC_OK;
}

int esc_get_environment_res(esc_context *ctx, int32_t *res) {
  if (!ctx || !res) {
    set_error(!ctx ? "esc_get_environment_res: ctx is null" : "esc_get_environment_res: res is null");
    return ESC_ERR_INVALID;
  }
  *res = ctx->env_res;
  return ESC_OK;
}

int esc_environment_sky(int32_t res, const float zenith[3], const float horizon[3], const float ground[3],
                        float *out) {
  const char *fn = "esc_environment_sky";
  if (res < 1 || res > esc::kEnvMaxRes) {
    set_error(std::string(fn) + ": res must be in 1..1024");
    return ESC_ERR_INVALID;
  }
  if (!zenith || !horizon || !ground || !out) {
    set_error(std::string(fn) + ": zenith, horizon, ground and out are required");
    return ESC_ERR_INVALID;
  }
  const double R = (double)res;
  for (int face = 0; face < 6; ++face) {
    const int axis = face / 2;
    for (int j = 0; j < res; ++j)
      for (int i = 0; i < res; ++i) {
        double D[3];
        D[axis] = (face & 1) ? -1.0 : 1.0;
        D[(axis + 1) % 3] = (((double)i + 0.5) / R) * 2.0 - 1.0;
        D[(axis + 2) % 3] = (((double)j + 0.5) / R) * 2.0 - 1.0;
        const double e = D[1] / std::sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
        float *o = out + 3 * (((size_t)face * res + j) * res + i);
        for (int c = 0; c < 3; ++c) {
          const double h = (double)horizon[c];
          o[c] = (float)(e >= 0.0 ? h + ((double)zenith[c] - h) * e : h + ((double)ground[c] - h) * (-e));
        }
      }
  }
  return ESC_OK;
}

int esc_environment_rays(esc_context *ctx, int64_t n, const float *d_dirs, float *d_rgb, uint8_t *d_rgb8) {
  const std::string fn("esc_environment_rays");
  if (!ctx) {
    set_error(fn + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if (!ctx->d_env) {
    set_error(fn + ": no environment (esc_set_environment)");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error(fn + ": n < 0");
    return ESC_ERR_INVALID;
  }
  if (n > 0 && (!d_dirs || (!d_rgb && !d_rgb8))) {
    set_error(fn + ": d_dirs and one of d_rgb, d_rgb8 are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_dirs | (uintptr_t)d_rgb) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned (d_rgb8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error(fn + ": n exceeds one launch (2^32 - 1 workgroups of 256 directions)");
    return ESC_ERR_INVALID;
  }
  if (n == 0) return ESC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  esc::EnvRaysParams p;
  std::memset(&p, 0, sizeof(p));
  p.env.texels = ctx->d_env;
  p.env.res = ctx->env_res;
  p.n = n;
  p.dirs = d_dirs;
  p.rgb = d_rgb;
  p.rgb8 = d_rgb8;
  const int e = esc_launch_environment_rays(&p, ctx->stream);
  if (e) {
    set_error(fn + ": k_environment_rays launch: " + hipGetErrorString((hipError_t)e));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_environment_lookup_host(int32_t res, const float *texels, int64_t n, const float *dirs, float *rgb) {
  const char *fn = "esc_environment_lookup_host";
  if (res < 1 || res > esc::kEnvMaxRes) {
    set_error(std::string(fn) + ": res must be in 1..1024");
    return ESC_ERR_INVALID;
  }
  if (n < 0 || !texels || (n > 0 && (!dirs || !rgb))) {
    set_error(std::string(fn) + ": n >= 0, texels, dirs and rgb are required");
    return ESC_ERR_INVALID;
  }
  std::vector<esc::EnvTexel> packed; // the records the kernels read, and rt_environ.h's code on them
  env_repack(res, texels, packed);
  for (int64_t i = 0; i < n; ++i)
    esc::env_lookup(packed.data(), res, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], rgb[3 * i], rgb[3 * i + 1],
                    rgb[3 * i + 2]);
  return ESC_OK;
}

// ---- ambient occlusion (rt_ambient.hip) ------------------------------------------------------------
int esc_ambient_cosine_table(int32_t sets, int32_t samples, uint64_t seed, float *out) {
  const char *fn = "esc_ambient_cosine_table";
  if (sets < 1 || sets > esc::kAmbientMaxDim || samples < 1 || samples > esc::kAmbientMaxDim) {
    set_error(std::string(fn) + ": sets and samples must be in 1..64");
    return ESC_ERR_INVALID;
  }
  if (!out) {
    set_error(std::string(fn) + ": out is null");
    return ESC_ERR_INVALID;
  }
  // splitmix64 from (seed, sets, samples); u = (x >> 11 + 1/2) * 2^-53 in (0, 1).  Malley's method: a
  // uniform point of the unit disc lifted to the hemisphere is cosine-weighted.
  uint64_t st = seed ^ ((uint64_t)sets << 48) ^ ((uint64_t)samples << 40);
  auto next = [&st]() {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return ((double)(z >> 11) + 0.5) * 0x1p-53;
  };
  const double two_pi = 6.283185307179586476925286766559;
  for (int64_t j = 0; j < (int64_t)sets * samples; ++j) {
    const double u1 = next(), u2 = next();
    const double r = std::sqrt(u1), phi = two_pi * u2;
    double v[3] = {r * std::cos(phi), r * std::sin(phi), std::sqrt(1.0 - u1)};
    const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int c = 0; c < 3; ++c) out[3 * j + c] = (float)(v[c] / len);
  }
  return ESC_OK;
}

int esc_set_ambient_table(esc_context *ctx, int32_t sets, int32_t samples, const float *host_table) {
  const char *fn = "esc_set_ambient_table";
  if (!ctx) {
    set_error(std::string(fn) + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if (sets < 1 || sets > esc::kAmbientMaxDim || samples < 1 || samples > esc::kAmbientMaxDim) {
    set_error(std::string(fn) + ": sets and samples must be in 1..64");
    return ESC_ERR_INVALID;
  }
  if (!host_table) {
    set_error(std::string(fn) + ": host_table is null");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // a call in flight may still read the old table
  const size_t bytes = (size_t)sets * samples * 3 * sizeof(float);
  ctx->am_sets = ctx->am_samples = 0;
  if (ctx->call.alloc(ctx->d_am_table, bytes / sizeof(float))) return ESC_ERR_HIP;
  HIP_TRY(hipMemcpyAsync(ctx->d_am_table, host_table, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream)); // host_table is the caller's again
  ctx->am_sets = sets;
  ctx->am_samples = samples;
  return ESC_OK;
}

// the checks esc_ambient_rays and esc_render_ambient share, after ctx and opts are known not to be null
static int ambient_options_ok(const esc_context *ctx, const char *fn_, const esc_ambient_options *o) {
  const std::string fn(fn_);
  if (!ctx->have_scene) {
    set_error(fn + ": no scene uploaded (esc_upload_scene / esc_upload_flat)");
    return ESC_ERR_INVALID;
  }
  if (!ctx->d_am_table) {
    set_error(fn + ": no sample table (esc_set_ambient_table)");
    return ESC_ERR_INVALID;
  }
  if (o->samples < 1 || o->samples > ctx->am_samples) {
    set_error(fn + ": samples must be in 1 .. the table's samples per set");
    return ESC_ERR_INVALID;
  }
  if (o->sets < 1 || o->sets > ctx->am_sets) {
    set_error(fn + ": sets must be in 1 .. the table's sets");
    return ESC_ERR_INVALID;
  }
  if (!(o->radius > 0.f) || !std::isfinite(o->radius)) {
    set_error(fn + ": radius must be a finite number > 0 (FLT_MAX: unbounded)");
    return ESC_ERR_INVALID;
  }
  if (!(o->bias >= 0.f) || !std::isfinite(o->bias)) {
    set_error(fn + ": bias must be a finite number >= 0");
    return ESC_ERR_INVALID;
  }
  if (o->flags & ~(uint32_t)ESC_RENDER_EXACT_ONLY) {
    set_error(fn + ": flags takes 0 or ESC_RENDER_EXACT_ONLY only");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

// k_ambient on n rays of an already validated call: the caller's arrays, or (cam != nullptr) the frame's.
// sky: the SKY instantiation, which also writes d_sky / d_light from the context's environment.
static int ambient_launch(esc_context *ctx, const char *fn, int64_t n, const float *d_origins, const float *d_dirs,
                          const esc_camera *cam, int32_t W, int32_t H, const esc_ambient_options *o,
                          uint32_t pixel_base, float *d_vis, int32_t *d_count, float *d_t, int32_t *d_geom,
                          int32_t *d_prim, bool sky = false, float *d_sky = nullptr, float *d_light = nullptr) {
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->d_amstats && ctx->call.alloc(ctx->d_amstats, esc::kAmbientStats)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_amstats, 0, esc::kAmbientStats * sizeof(unsigned long long), ctx->stream));
  ctx->am_k = o->samples;
  if (n == 0) return ESC_OK;
  esc::AmbientParams p;
  std::memset(&p, 0, sizeof(p));
  p.q.n = n;
  p.q.orig = d_origins;
  p.q.dir = d_dirs;
  query_tables(ctx, p.q);
  p.q.exact_only = (o->flags & ESC_RENDER_EXACT_ONLY) ? 1 : 0;
  p.vis = d_vis;
  p.count = d_count;
  p.t = d_t;
  p.geom = d_geom;
  p.prim = d_prim;
  p.tri_n = ctx->d_tri_n;
  p.mat = ctx->d_mat;
  p.table = ctx->d_am_table;
  p.samples = o->samples;
  p.sets = o->sets;
  p.row_samples = ctx->am_samples;
  p.radius = o->radius;
  p.bias = o->bias;
  p.seed = o->seed;
  p.pixel_base = pixel_base;
  if (sky) {
    p.env.texels = ctx->d_env;
    p.env.res = ctx->env_res;
    p.sky = d_sky;
    p.light = d_light;
    p.sph_mat = ctx->d_sph_mat;
  }
  if (cam) {
    p.W = W;
    p.H = H;
    std::memcpy(p.origin, cam->origin, 12);
    std::memcpy(p.llc, cam->lower_left_corner, 12);
    std::memcpy(p.horizontal, cam->horizontal, 12);
    std::memcpy(p.vertical, cam->vertical, 12);
  }
  // ESC_AMBIENT_STATS=0: nothing is counted (the A/B of tools/ambient_time.py; the stats then read zero)
  const char *e = std::getenv("ESC_AMBIENT_STATS");
  p.stats = (e && e[0] == '0') ? nullptr : ctx->d_amstats;
  const int rc = esc_launch_ambient(&p, cam ? 1 : 0, sky ? 1 : 0, ctx->stream);
  if (rc) {
    set_error(std::string(fn) + ": k_ambient launch: " + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_ambient_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                     const esc_ambient_options *opts, float *d_vis, int32_t *d_count, float *d_t,
                     int32_t *d_geom, int32_t *d_prim) {
  const char *fn = "esc_ambient_rays";
  if (!ctx || !opts) {
    set_error(!ctx ? "esc_ambient_rays: ctx is null" : "esc_ambient_rays: opts is null");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error("esc_ambient_rays: n < 0");
    return ESC_ERR_INVALID;
  }
  const int rc = ambient_options_ok(ctx, fn, opts);
  if (rc) return rc;
  if (n > 0 && (!d_origins || !d_dirs || !d_vis)) {
    set_error("esc_ambient_rays: d_origins, d_dirs and d_vis are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_vis | (uintptr_t)d_count | (uintptr_t)d_t |
       (uintptr_t)d_geom | (uintptr_t)d_prim) & 3u) {
    set_error("esc_ambient_rays: device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_ambient_rays: n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  return ambient_launch(ctx, fn, n, d_origins, d_dirs, nullptr, 0, 0, opts, opts->pixel_base, d_vis, d_count, d_t,
                        d_geom, d_prim);
}

int esc_render_ambient(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                       const esc_ambient_options *opts, float *d_vis, int32_t *d_count) {
  const char *fn_ = "esc_render_ambient";
  const std::string fn(fn_);
  if (!ctx || !cam || !opts || !d_vis) {
    set_error(!ctx ? fn + ": ctx is null" : !opts ? fn + ": opts is null" : fn + ": cam or d_vis is null");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error(fn + ": need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  if ((int64_t)W * H > 0x7fffffffLL) {
    set_error(fn + ": W*H exceeds the reference's int pixel index (main.cpp:784)");
    return ESC_ERR_INVALID;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->lower_left_corner[k]) ||
        !std::isfinite(cam->horizontal[k]) || !std::isfinite(cam->vertical[k])) {
      set_error(fn + ": camera is not finite");
      return ESC_ERR_INVALID;
    }
  const int rc = ambient_options_ok(ctx, fn_, opts);
  if (rc) return rc;
  if (((uintptr_t)d_vis | (uintptr_t)d_count) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  return ambient_launch(ctx, fn_, (int64_t)W * H, nullptr, nullptr, cam, W, H, opts, 0u, d_vis, d_count, nullptr,
                        nullptr, nullptr);
}

// ---- sky lighting (rt_ambient.hip with SKY) -----------------------------------------
// ambient_options_ok plus the environment the SKY kernels read
static int skylight_options_ok(const esc_context *ctx, const char *fn, const esc_ambient_options *o) {
  const int rc = ambient_options_ok(ctx, fn, o);
  if (rc) return rc;
  if (!ctx->d_env) {
    set_error(std::string(fn) + ": no environment (esc_set_environment)");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

int esc_skylight_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs,
                      const esc_ambient_options *opts, float *d_sky, float *d_light, float *d_vis,
                      int32_t *d_count, float *d_t, int32_t *d_geom, int32_t *d_prim) {
  const char *fn_ = "esc_skylight_rays";
  const std::string fn(fn_);
  if (!ctx || !opts) {
    set_error(!ctx ? fn + ": ctx is null" : fn + ": opts is null");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error(fn + ": n < 0");
    return ESC_ERR_INVALID;
  }
  const int rc = skylight_options_ok(ctx, fn_, opts);
  if (rc) return rc;
  if (n > 0 && (!d_origins || !d_dirs || (!d_sky && !d_light))) {
    set_error(fn + ": d_origins, d_dirs and one of d_sky, d_light are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_sky | (uintptr_t)d_light | (uintptr_t)d_vis |
       (uintptr_t)d_count | (uintptr_t)d_t | (uintptr_t)d_geom | (uintptr_t)d_prim) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error(fn + ": n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  return ambient_launch(ctx, fn_, n, d_origins, d_dirs, nullptr, 0, 0, opts, opts->pixel_base, d_vis, d_count, d_t,
                        d_geom, d_prim, true, d_sky, d_light);
}

int esc_render_skylight(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                        const esc_ambient_options *opts, float *d_sky, float *d_light, float *d_vis,
                        int32_t *d_count) {
  const char *fn_ = "esc_render_skylight";
  const std::string fn(fn_);
  if (!ctx || !cam || !opts || (!d_sky && !d_light)) {
    set_error(!ctx    ? fn + ": ctx is null"
              : !opts ? fn + ": opts is null"
              : !cam  ? fn + ": cam is null"
                      : fn + ": one of d_sky, d_light is required");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error(fn + ": need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  if ((int64_t)W * H > 0x7fffffffLL) {
    set_error(fn + ": W*H exceeds the reference's int pixel index (main.cpp:784)");
    return ESC_ERR_INVALID;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->lower_left_corner[k]) ||
        !std::isfinite(cam->horizontal[k]) || !std::isfinite(cam->vertical[k])) {
      set_error(fn + ": camera is not finite");
      return ESC_ERR_INVALID;
    }
  const int rc = skylight_options_ok(ctx, fn_, opts);
  if (rc) return rc;
  if (((uintptr_t)d_sky | (uintptr_t)d_light | (uintptr_t)d_vis | (uintptr_t)d_count) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  return ambient_launch(ctx, fn_, (int64_t)W * H, nullptr, nullptr, cam, W, H, opts, 0u, d_vis, d_count, nullptr,
                        nullptr, nullptr, true, d_sky, d_light);
}

int esc_add_light(esc_context *ctx, int64_t n, const float *d_rgb, const float *d_light, float *d_out,
                  uint8_t *d_out8) {
  if (!ctx) {
    set_error("esc_add_light: ctx is null");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error("esc_add_light: n < 0");
    return ESC_ERR_INVALID;
  }
  if (n > 0 && (!d_rgb || !d_light || (!d_out && !d_out8))) {
    set_error("esc_add_light: d_rgb, d_light and one of d_out, d_out8 are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_rgb | (uintptr_t)d_light | (uintptr_t)d_out) & 3u) {
    set_error("esc_add_light: device pointers must be 4-byte aligned (d_out8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_add_light: n exceeds one launch (2^32 - 1 workgroups of 256 pixels)");
    return ESC_ERR_INVALID;
  }
  if (n == 0) return ESC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  esc::AddLightParams p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.rgb = d_rgb;
  p.light = d_light;
  p.out = d_out;
  p.out8 = d_out8;
  const int rc = esc_launch_add_light(&p, ctx->stream);
  if (rc) {
    set_error(std::string("esc_add_light: k_add_light launch: ") + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_modulate(esc_context *ctx, int64_t n, const float *d_rgb, const float *d_vis, float *d_out,
                 uint8_t *d_out8) {
  if (!ctx) {
    set_error("esc_modulate: ctx is null");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error("esc_modulate: n < 0");
    return ESC_ERR_INVALID;
  }
  if (n > 0 && (!d_rgb || !d_vis || (!d_out && !d_out8))) {
    set_error("esc_modulate: d_rgb, d_vis and one of d_out, d_out8 are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_rgb | (uintptr_t)d_vis | (uintptr_t)d_out) & 3u) {
    set_error("esc_modulate: device pointers must be 4-byte aligned (d_out8 excepted)");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error("esc_modulate: n exceeds one launch (2^32 - 1 workgroups of 256 pixels)");
    return ESC_ERR_INVALID;
  }
  if (n == 0) return ESC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  esc::ModulateParams p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.rgb = d_rgb;
  p.vis = d_vis;
  p.out = d_out;
  p.out8 = d_out8;
  const int rc = esc_launch_modulate(&p, ctx->stream);
  if (rc) {
    set_error(std::string("esc_modulate: k_modulate launch: ") + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_last_ambient_stats(esc_context *ctx, esc_ambient_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_ambient_stats: ctx is null" : "esc_last_ambient_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kAmbientStats] = {0, 0, 0, 0, 0};
  if (ctx->d_amstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_amstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->rays = h[0];
  out->hit_rays = h[1];
  out->samples = h[1] * (uint64_t)ctx->am_k;
  out->occluded_samples = h[2];
  out->exact_rays = h[3];
  out->exact_tests = h[4];
  return ESC_OK;
}

// ---- the G-buffer of rays and frames (rt_gbuffer.hip) -------------------------------
// k_gbuffer on n rays of an already validated call: the caller's arrays, or (cam != nullptr) the frame's
static int gbuffer_launch(esc_context *ctx, const char *fn, int64_t n, const float *d_origins, const float *d_dirs,
                          const esc_camera *cam, int32_t W, int32_t H, uint32_t flags, float *d_normal,
                          float *d_position, float *d_albedo, float *d_t, int32_t *d_geom, int32_t *d_prim) {
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->d_gbstats && ctx->call.alloc(ctx->d_gbstats, esc::kGBufferStats)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_gbstats, 0, esc::kGBufferStats * sizeof(unsigned long long), ctx->stream));
  if (n == 0) return ESC_OK;
  esc::GBufferParams p;
  std::memset(&p, 0, sizeof(p));
  p.q.n = n;
  p.q.orig = d_origins;
  p.q.dir = d_dirs;
  query_tables(ctx, p.q);
  p.q.exact_only = (flags & ESC_RENDER_EXACT_ONLY) ? 1 : 0;
  p.normal = d_normal;
  p.position = d_position;
  p.albedo = d_albedo;
  p.t = d_t;
  p.geom = d_geom;
  p.prim = d_prim;
  p.tri_n = ctx->d_tri_n;
  p.mat = ctx->d_mat;
  p.sph_mat = ctx->d_sph_mat;
  if (cam) {
    p.W = W;
    p.H = H;
    std::memcpy(p.origin, cam->origin, 12);
    std::memcpy(p.llc, cam->lower_left_corner, 12);
    std::memcpy(p.horizontal, cam->horizontal, 12);
    std::memcpy(p.vertical, cam->vertical, 12);
  }
  p.stats = ctx->d_gbstats;
  const int rc = esc_launch_gbuffer(&p, cam ? 1 : 0, ctx->stream);
  if (rc) {
    set_error(std::string(fn) + ": k_gbuffer launch: " + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

// the checks esc_gbuffer_rays and esc_render_gbuffer share, after ctx is known not to be null
static int gbuffer_args_ok(const esc_context *ctx, const std::string &fn, int64_t n, uint32_t flags,
                           const void *d_normal, const void *d_position, const void *d_albedo, const void *d_t,
                           const void *d_geom, const void *d_prim) {
  if (!ctx->have_scene) {
    set_error(fn + ": no scene uploaded (esc_upload_scene / esc_upload_flat)");
    return ESC_ERR_INVALID;
  }
  if (flags & ~(uint32_t)ESC_RENDER_EXACT_ONLY) {
    set_error(fn + ": flags takes 0 or ESC_RENDER_EXACT_ONLY only");
    return ESC_ERR_INVALID;
  }
  if (n > 0 && !d_normal && !d_position && !d_albedo && !d_t && !d_geom && !d_prim) {
    set_error(fn + ": one of d_normal, d_position, d_albedo, d_t, d_geom, d_prim is required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_normal | (uintptr_t)d_position | (uintptr_t)d_albedo | (uintptr_t)d_t | (uintptr_t)d_geom |
       (uintptr_t)d_prim) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  return ESC_OK;
}

int esc_gbuffer_rays(esc_context *ctx, int64_t n, const float *d_origins, const float *d_dirs, uint32_t flags,
                     float *d_normal, float *d_position, float *d_albedo, float *d_t, int32_t *d_geom,
                     int32_t *d_prim) {
  const char *fn_ = "esc_gbuffer_rays";
  const std::string fn(fn_);
  if (!ctx) {
    set_error(fn + ": ctx is null");
    return ESC_ERR_INVALID;
  }
  if (n < 0) {
    set_error(fn + ": n < 0");
    return ESC_ERR_INVALID;
  }
  const int rc = gbuffer_args_ok(ctx, fn, n, flags, d_normal, d_position, d_albedo, d_t, d_geom, d_prim);
  if (rc) return rc;
  if (n > 0 && (!d_origins || !d_dirs)) {
    set_error(fn + ": d_origins and d_dirs are required");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_origins | (uintptr_t)d_dirs) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  if (n > (int64_t)0xffffffffu * 256) {
    set_error(fn + ": n exceeds one launch (2^32 - 1 workgroups of 256 rays)");
    return ESC_ERR_INVALID;
  }
  return gbuffer_launch(ctx, fn_, n, d_origins, d_dirs, nullptr, 0, 0, flags, d_normal, d_position, d_albedo, d_t,
                        d_geom, d_prim);
}

int esc_render_gbuffer(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H, uint32_t flags,
                       float *d_normal, float *d_position, float *d_albedo, float *d_t, int32_t *d_geom,
                       int32_t *d_prim) {
  const char *fn_ = "esc_render_gbuffer";
  const std::string fn(fn_);
  if (!ctx || !cam) {
    set_error(!ctx ? fn + ": ctx is null" : fn + ": cam is null");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error(fn + ": need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  if ((int64_t)W * H > 0x7fffffffLL) {
    set_error(fn + ": W*H exceeds the reference's int pixel index (main.cpp:784)");
    return ESC_ERR_INVALID;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->lower_left_corner[k]) ||
        !std::isfinite(cam->horizontal[k]) || !std::isfinite(cam->vertical[k])) {
      set_error(fn + ": camera is not finite");
      return ESC_ERR_INVALID;
    }
  const int rc =
      gbuffer_args_ok(ctx, fn, (int64_t)W * H, flags, d_normal, d_position, d_albedo, d_t, d_geom, d_prim);
  if (rc) return rc;
  return gbuffer_launch(ctx, fn_, (int64_t)W * H, nullptr, nullptr, cam, W, H, flags, d_normal, d_position,
                        d_albedo, d_t, d_geom, d_prim);
}

int esc_last_gbuffer_stats(esc_context *ctx, esc_gbuffer_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_gbuffer_stats: ctx is null" : "esc_last_gbuffer_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kGBufferStats] = {0, 0, 0, 0};
  if (ctx->d_gbstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_gbstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->rays = h[0];
  out->hit_rays = h[1];
  out->exact_rays = h[2];
  out->exact_tests = h[3];
  return ESC_OK;
}

// ---- the edge-stopping a-trous filter (rt_filter.hip) -------------------------------
int esc_filter_guided(esc_context *ctx, int32_t W, int32_t H, int32_t channels, const float *d_in,
                      const float *d_normal, const float *d_position, const int32_t *d_geom, const int32_t *d_prim,
                      const esc_filter_options *opts, float *d_out) {
  const std::string fn("esc_filter_guided");
  if (!ctx || !opts) {
    set_error(!ctx ? fn + ": ctx is null" : fn + ": opts is null");
    return ESC_ERR_INVALID;
  }
  if (W < 1 || H < 1) {
    set_error(fn + ": need W,H >= 1");
    return ESC_ERR_INVALID;
  }
  if (channels != 1 && channels != 3) {
    set_error(fn + ": channels must be 1 or 3");
    return ESC_ERR_INVALID;
  }
  if (opts->iterations < 1 || opts->iterations > esc::kFilterMaxIter) {
    set_error(fn + ": iterations must be in 1 .. 8");
    return ESC_ERR_INVALID;
  }
  if (std::isnan(opts->normal_cos)) {
    set_error(fn + ": normal_cos must not be NaN");
    return ESC_ERR_INVALID;
  }
  if (!(opts->plane_dist >= 0.f)) {
    set_error(fn + ": plane_dist must be >= 0 and not NaN (FLT_MAX or inf: off)");
    return ESC_ERR_INVALID;
  }
  if (opts->same_object != 0 && opts->same_object != 1) {
    set_error(fn + ": same_object must be 0 or 1");
    return ESC_ERR_INVALID;
  }
  if (opts->reserved[0] || opts->reserved[1]) {
    set_error(fn + ": reserved must be 0");
    return ESC_ERR_INVALID;
  }
  if (!d_in || !d_normal || !d_position || !d_geom || !d_prim || !d_out) {
    set_error(fn + ": d_in, d_normal, d_position, d_geom, d_prim and d_out are required");
    return ESC_ERR_INVALID;
  }
  if (d_in == d_out) {
    set_error(fn + ": d_out must not be d_in");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_in | (uintptr_t)d_normal | (uintptr_t)d_position | (uintptr_t)d_geom | (uintptr_t)d_prim |
       (uintptr_t)d_out) & 3u) {
    set_error(fn + ": device pointers must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  const int64_t n = (int64_t)W * H;
  const int64_t tiles_x = ((int64_t)W + esc::kFilterTileW - 1) / esc::kFilterTileW;
  const int64_t tiles = tiles_x * (((int64_t)H + esc::kFilterTileH - 1) / esc::kFilterTileH);
  if (tiles > (int64_t)0x7fffffff || n > (int64_t)0xffffffffu * 256) {
    set_error(fn + ": W*H exceeds one launch (2^31 - 1 tiles of 64 x 4 pixels)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->d_flstats && ctx->call.alloc(ctx->d_flstats, esc::kFilterStats)) return ESC_ERR_HIP;
  const int L = opts->iterations;
  if (ctx->call.grow(ctx->d_fl_guide, ctx->fl_guide_cap, (size_t)n)) return ESC_ERR_HIP;
  if (L > 1 && ctx->call.grow(ctx->d_fl_img, ctx->fl_img_cap, (size_t)n * (size_t)channels)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_flstats, 0, esc::kFilterStats * sizeof(unsigned long long), ctx->stream));
  ctx->fl_pixels = (uint64_t)n;
  esc::FilterPackParams k;
  std::memset(&k, 0, sizeof(k));
  k.n = n;
  k.normal = d_normal;
  k.position = d_position;
  k.geom = d_geom;
  k.prim = d_prim;
  k.guide = ctx->d_fl_guide;
  k.stats = ctx->d_flstats;
  int rc = esc_launch_filter_pack(&k, ctx->stream);
  if (rc) {
    set_error(fn + ": k_filter_pack launch: " + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  esc::FilterParams p;
  std::memset(&p, 0, sizeof(p));
  p.W = W;
  p.H = H;
  p.same_object = opts->same_object;
  p.normal_cos = opts->normal_cos;
  p.plane_dist = opts->plane_dist;
  p.tiles_x = tiles_x;
  p.guide = ctx->d_fl_guide;
  p.stats = ctx->d_flstats;
  // the last iteration lands in d_out: iteration i writes d_out when L - 1 - i is even, else the scratch
  const float *src = d_in;
  for (int i = 0; i < L; i++) {
    float *dst = ((L - 1 - i) & 1) ? ctx->d_fl_img : d_out;
    p.step = 1 << i;
    p.in = src;
    p.out = dst;
    rc = esc_launch_filter_atrous(&p, channels, tiles, ctx->stream);
    if (rc) {
      set_error(fn + ": k_filter_atrous launch: " + hipGetErrorString((hipError_t)rc));
      return ESC_ERR_HIP;
    }
    src = dst;
  }
  return ESC_OK;
}

int esc_last_filter_stats(esc_context *ctx, esc_filter_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_filter_stats: ctx is null" : "esc_last_filter_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kFilterStats] = {0, 0, 0};
  if (ctx->d_flstats) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h, ctx->d_flstats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->pixels = ctx->d_flstats ? ctx->fl_pixels : 0;
  out->hit_pixels = h[0];
  out->taps_tested = h[1];
  out->taps_accepted = h[2];
  return ESC_OK;
}

// ---- temporal accumulation (rt_temporal.hip) -----------------------------------------
int esc_temporal_accumulate(esc_context *ctx, const esc_camera *prev_cam, int32_t W, int32_t H, int32_t channels,
                            const float *d_current, const esc_guides *cur, const float *d_history,
                            const int32_t *d_history_n, const esc_guides *prev, const esc_temporal_options *opts,
                            float *d_out, int32_t *d_out_n) {
  const std::string fn("esc_temporal_accumulate");
  if (!ctx || !opts || !prev_cam || !cur || !prev) {
    set_error(fn + (!ctx ? ": ctx is null" : !opts ? ": opts is null" : !prev_cam ? ": prev_cam is null"
                    : !cur ? ": cur is null" : ": prev is null"));
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error(fn + ": need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  if (channels != 1 && channels != 3) {
    set_error(fn + ": channels must be 1 or 3");
    return ESC_ERR_INVALID;
  }
  if (opts->taps != 1 && opts->taps != 4) {
    set_error(fn + ": taps must be 1 or 4");
    return ESC_ERR_INVALID;
  }
  if (opts->max_history < 1 || opts->max_history > esc::kTemporalMaxHistory) {
    set_error(fn + ": max_history must be in 1 .. 65536");
    return ESC_ERR_INVALID;
  }
  if (std::isnan(opts->normal_cos)) {
    set_error(fn + ": normal_cos must not be NaN");
    return ESC_ERR_INVALID;
  }
  if (!(opts->plane_dist >= 0.f)) {
    set_error(fn + ": plane_dist must be >= 0 and not NaN (FLT_MAX or inf: off)");
    return ESC_ERR_INVALID;
  }
  if (opts->same_object != 0 && opts->same_object != 1) {
    set_error(fn + ": same_object must be 0 or 1");
    return ESC_ERR_INVALID;
  }
  if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2]) {
    set_error(fn + ": reserved must be 0");
    return ESC_ERR_INVALID;
  }
  if (!d_current || !d_history || !d_history_n || !d_out || !d_out_n) {
    set_error(fn + ": d_current, d_history, d_history_n, d_out and d_out_n are required");
    return ESC_ERR_INVALID;
  }
  for (int k = 0; k < 2; k++) {
    const esc_guides *g = k ? prev : cur;
    if (!g->normal || !g->position || !g->geom || !g->prim) {
      set_error(fn + (k ? ": prev" : ": cur") + "'s normal, position, geom and prim are required");
      return ESC_ERR_INVALID;
    }
    if (((uintptr_t)g->normal | (uintptr_t)g->position | (uintptr_t)g->geom | (uintptr_t)g->prim) & 3u) {
      set_error(fn + (k ? ": prev" : ": cur") + "'s device pointers must be 4-byte aligned");
      return ESC_ERR_INVALID;
    }
  }
  if (d_out == d_history) {
    set_error(fn + ": d_out must not be d_history");
    return ESC_ERR_INVALID;
  }
  if (d_out_n == d_history_n) {
    set_error(fn + ": d_out_n must not be d_history_n");
    return ESC_ERR_INVALID;
  }
  if (((uintptr_t)d_current | (uintptr_t)d_history | (uintptr_t)d_history_n | (uintptr_t)d_out |
       (uintptr_t)d_out_n) & 3u) {
    set_error(fn + ": d_current, d_history, d_history_n, d_out and d_out_n must be 4-byte aligned");
    return ESC_ERR_INVALID;
  }
  const int64_t tiles_x = ((int64_t)W + esc::kTemporalTileW - 1) / esc::kTemporalTileW;
  const int64_t tiles = tiles_x * (((int64_t)H + esc::kTemporalTileH - 1) / esc::kTemporalTileH);
  if (tiles > (int64_t)0x7fffffff) {
    set_error(fn + ": W*H exceeds one launch (2^31 - 1 tiles of 64 x 4 pixels)");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->d_tpstats && ctx->call.alloc(ctx->d_tpstats, (size_t)esc::kTemporalStatSets * 8)) return ESC_ERR_HIP;
  HIP_TRY(hipMemsetAsync(ctx->d_tpstats, 0, esc::kTemporalStatSets * 8 * sizeof(unsigned long long), ctx->stream));
  ctx->tp_pixels = (uint64_t)W * (uint64_t)H;
  esc::TemporalParams p;
  std::memset(&p, 0, sizeof(p));
  p.W = W;
  p.H = H;
  p.same_object = opts->same_object;
  p.max_history = opts->max_history;
  p.normal_cos = opts->normal_cos;
  p.plane_dist = opts->plane_dist;
  for (int k = 0; k < 3; k++) {
    p.origin[k] = prev_cam->origin[k];
    p.lower_left_corner[k] = prev_cam->lower_left_corner[k];
    p.horizontal[k] = prev_cam->horizontal[k];
    p.vertical[k] = prev_cam->vertical[k];
  }
  p.tiles_x = tiles_x;
  p.current = d_current;
  p.cur = {cur->normal, cur->position, cur->geom, cur->prim};
  p.prev = {prev->normal, prev->position, prev->geom, prev->prim};
  p.history = d_history;
  p.history_n = d_history_n;
  p.out = d_out;
  p.out_n = d_out_n;
  p.stats = ctx->d_tpstats;
  const int rc = esc_launch_temporal(&p, channels, opts->taps, tiles, ctx->stream);
  if (rc) {
    set_error(fn + ": k_temporal launch: " + hipGetErrorString((hipError_t)rc));
    return ESC_ERR_HIP;
  }
  return ESC_OK;
}

int esc_last_temporal_stats(esc_context *ctx, esc_temporal_stats *out) {
  if (!ctx || !out) {
    set_error(!ctx ? "esc_last_temporal_stats: ctx is null" : "esc_last_temporal_stats: out is null");
    return ESC_ERR_INVALID;
  }
  unsigned long long h[esc::kTemporalStats] = {0, 0, 0, 0};
  if (ctx->d_tpstats) {
    unsigned long long all[esc::kTemporalStatSets * 8];
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(all, ctx->d_tpstats, sizeof(all), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < esc::kTemporalStatSets; s++)
      for (int j = 0; j < esc::kTemporalStats; j++) h[j] += all[s * 8 + j];
  }
  out->pixels = ctx->d_tpstats ? ctx->tp_pixels : 0;
  out->hit_pixels = h[0];
  out->reused_pixels = h[1];
  out->taps_tested = h[2];
  out->taps_accepted = h[3];
  return ESC_OK;
}

int esc_live_device_allocations(int64_t *buffers, int64_t *bytes) {
  if (buffers) *buffers = g_live_buffers.load();
  if (bytes) *bytes = g_live_bytes.load();
  return ESC_OK;
}

int esc_reset_counters(esc_context *ctx) {
  if (!ctx) {
    set_error("esc_reset_counters: ctx is null");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, esc::kCounterSets * 8 * sizeof(unsigned long long), ctx->stream));
  return ESC_OK;
}

int esc_read_counters(esc_context *ctx, esc_counters *out) {
  if (!ctx || !out) {
    set_error("esc_read_counters: bad argument");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  unsigned long long all[esc::kCounterSets * 8];
  HIP_TRY(hipMemcpyAsync(all, ctx->d_counters, sizeof(all), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  unsigned long long h[5] = {0, 0, 0, 0, 0};
  for (int s = 0; s < esc::kCounterSets; s++)
    for (int j = 0; j < 5; j++) h[j] += all[s * 8 + j];
  out->primary_rays = h[0];
  out->hit_pixels = h[1];
  out->shadow_rays = h[2];
  out->anyhit_tests = h[3];
  out->anyhit_lane_tests = h[4];
  return ESC_OK;
}

int esc_render_frame_host(esc_context *ctx, const esc_camera *cam, int32_t W, int32_t H,
                          const esc_render_options *opts, float *image, uint8_t *rgb8) {
  if (!ctx || (!image && !rgb8)) {
    set_error("esc_render_frame_host: bad argument");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error("esc_render_frame_host: need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)W * H * 3;
  int rc;
  if (image && (rc = ctx->call.grow(ctx->d_img, ctx->img_cap, n))) return rc;
  if (rgb8 && (rc = ctx->call.grow(ctx->d_u8, ctx->u8_cap, n))) return rc;
  rc = esc_render_rows(ctx, cam, W, H, 0, H, opts, image ? ctx->d_img : nullptr,
                           rgb8 ? ctx->d_u8 : nullptr);
  if (rc) return rc;
  if (image)
    HIP_TRY(hipMemcpyAsync(image, ctx->d_img, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (rgb8) HIP_TRY(hipMemcpyAsync(rgb8, ctx->d_u8, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ESC_OK;
}

int esc_render_frame_multi(const esc_scene *scene, const esc_camera *cam, int32_t W, int32_t H,
                           const esc_render_options *opts, int32_t n_devices, float *image,
                           uint8_t *rgb8, float *ms_per_device) {
  if (!scene || !cam || !opts || n_devices < 1 || (!image && !rgb8)) {
    set_error("esc_render_frame_multi: bad argument");
    return ESC_ERR_INVALID;
  }
  if (W < 2 || H < 2) {
    set_error("esc_render_frame_multi: need W,H >= 2");
    return ESC_ERR_INVALID;
  }
  int avail = 0;
  if (hipGetDeviceCount(&avail) != hipSuccess || avail < 1) {
    set_error("esc_render_frame_multi: no HIP device (no CPU fallback)");
    return ESC_ERR_NO_DEVICE;
  }
  // 8-row strips dealt round-robin: band i renders strips i, i+n, ... (load balance, see
  // esc_render_strips) and each strip is copied straight to its rows of the caller's frame.
  const int kStrip = 8;
  struct Band {
    esc_context *ctx = nullptr;
    float *d_img = nullptr; // the band's rows, the context's call memory
    uint8_t *d_u8 = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    int rows = 0;
  };
  std::vector<Band> bands((size_t)n_devices);
  int rc = ESC_OK;
  auto cleanup = [&]() {
    for (auto &b : bands) {
      if (!b.ctx) continue;
      (void)hipSetDevice(b.ctx->device);
      if (b.t0) (void)hipEventDestroy(b.t0);
      if (b.t1) (void)hipEventDestroy(b.t1);
      esc_context_destroy(b.ctx);
    }
  };
#define MULTI_TRY(expr)                                                      \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
      cleanup();                                                             \
      return ESC_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)
  // phase 1: one context per band; bands beyond the device count share devices round-robin
  for (int i = 0; i < n_devices && rc == ESC_OK; i++) {
    Band &b = bands[(size_t)i];
    b.rows = esc_strip_local_rows(H, kStrip, i, n_devices);
    rc = esc_context_create(i % avail, &b.ctx);
    if (rc == ESC_OK) rc = esc_upload_scene(b.ctx, scene);
  }
  if (rc != ESC_OK) {
    cleanup();
    return rc;
  }
  // phase 2: launch every band before waiting on any
  const int n_strips = (H + kStrip - 1) / kStrip;
  for (int i = 0; i < n_devices; i++) {
    Band &b = bands[(size_t)i];
    if (b.rows == 0) continue;
    const size_t n = (size_t)b.rows * W * 3;
    MULTI_TRY(hipSetDevice(b.ctx->device));
    if (image) rc = b.ctx->call.alloc(b.d_img, n);
    if (rgb8 && rc == ESC_OK) rc = b.ctx->call.alloc(b.d_u8, n);
    if (rc != ESC_OK) {
      cleanup();
      return rc;
    }
    MULTI_TRY(hipEventCreate(&b.t0));
    MULTI_TRY(hipEventCreate(&b.t1));
    MULTI_TRY(hipEventRecord(b.t0, b.ctx->stream));
    rc = esc_render_strips(b.ctx, cam, W, H, kStrip, i, n_devices, opts, b.d_img, b.d_u8);
    if (rc != ESC_OK) {
      cleanup();
      return rc;
    }
    MULTI_TRY(hipEventRecord(b.t1, b.ctx->stream));
    // gather: strip k = image rows [k*8, k*8+8) sits at local rows [j*8, ...) of band i
    size_t local_row = 0;
    for (int k = i; k < n_strips; k += n_devices) {
      const int h0 = k * kStrip;
      const size_t rows = (size_t)std::min(kStrip, H - h0);
      const size_t cnt = rows * W * 3;
      if (image)
        MULTI_TRY(hipMemcpyAsync(image + (size_t)h0 * W * 3, b.d_img + local_row * W * 3,
                                 cnt * sizeof(float), hipMemcpyDeviceToHost, b.ctx->stream));
      if (rgb8)
        MULTI_TRY(hipMemcpyAsync(rgb8 + (size_t)h0 * W * 3, b.d_u8 + local_row * W * 3, cnt,
                                 hipMemcpyDeviceToHost, b.ctx->stream));
      local_row += rows;
    }
  }
  for (size_t i = 0; i < bands.size(); i++) {
    Band &b = bands[i];
    if (ms_per_device) ms_per_device[i] = 0.f;
    if (b.rows == 0) continue;
    MULTI_TRY(hipSetDevice(b.ctx->device));
    MULTI_TRY(hipStreamSynchronize(b.ctx->stream));
    if (ms_per_device) MULTI_TRY(hipEventElapsedTime(&ms_per_device[i], b.t0, b.t1));
  }
#undef MULTI_TRY
  cleanup();
  return ESC_OK;
}

// ---------------------------------------------------------------------------------------
// the ISPC drop-in (trace.ispc:86-92 / main.cpp:619-624)
// ---------------------------------------------------------------------------------------
void trace(int32_t image_width, int32_t image_height, ispc_cam *cam, int32_t num_triangles,
           ispc_triangle triangles[], int32_t num_lights, ispc_light lights[],
           int32_t num_light_triangles, ispc_triangle light_triangles[], float *return_image,
           int32_t debug, int32_t test) {
  (void)test; // accepted and ignored, like trace.ispc:92 (defect I6)
  if (!return_image || image_width <= 0 || image_height <= 0) return;
  const size_t n = (size_t)image_width * image_height * 3;
  std::memset(return_image, 0, n * sizeof(float)); // overwrite semantics (defect I3)
  static esc_context *ctx = nullptr; // one per process, like the single call site
  int rc = ESC_OK;
  if (!ctx) {
    const char *dev = std::getenv("ESC_DEVICE");
    rc = esc_context_create(dev ? std::atoi(dev) : 0, &ctx);
  }
  if (rc == ESC_OK)
    rc = esc_upload_flat(ctx, num_triangles, triangles, num_lights, lights, num_light_triangles,
                         light_triangles);
  if (rc == ESC_OK) {
    if (!cam) {
      set_error("trace: cam is null");
      rc = ESC_ERR_INVALID;
    }
  }
  if (rc == ESC_OK) {
    esc_camera c;
    esc_camera_init(&c, cam->lookfrom, cam->lookat, cam->vup, cam->vfov, cam->aspect);
    esc_render_options o;
    std::memset(&o, 0, sizeof(o));
    o.shadows = 1;
    o.face_mode = ESC_FACE_HASH; // == face 0 for single-face lights
    o.seed = 0;
    // the 12-argument seam has no room for options: $ESC_TRACE_STAGE=bvh opts into the tree
    const char *st = std::getenv("ESC_TRACE_STAGE");
    if (st && std::strcmp(st, "bvh") == 0) o.stage = ESC_STAGE_BVH;
    rc = esc_render_frame_host(ctx, &c, image_width, image_height, &o, return_image, nullptr);
  }
  if (rc != ESC_OK) {
    std::fprintf(stderr, "esctp1raytracer_amd trace(): error %d: %s\n", rc, esc_last_error());
    std::memset(return_image, 0, n * sizeof(float));
  } else if (debug >= 2) {
    std::fprintf(stderr, "esctp1raytracer_amd trace(): w=%d h=%d triangles=%d lights=%d\n",
                 image_width, image_height, num_triangles, num_lights);
  }
}

} // extern "C"
