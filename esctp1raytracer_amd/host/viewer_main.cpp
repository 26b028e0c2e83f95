// viewer_main.cpp -- ESCViewer2021: the reference's command line on top of the MI355X renderer.
//
// Keeps the surface of /root/reference/src/main.cpp:417-695 (flags at :430-535, timing print
// at :645-654, P3 PPM at :658-689, stdout messages at :688-691) and replaces what happens
// between "start the clock" and "stop the clock": every mode renders on the GPU through the
// C ABI (include/esctp1_rt.h).  Host C++ only talks to the library through that ABI.
//
//   -m model.obj  -o out.ppm  -v ex,ey,ez  -l lx,ly,lz      as the reference
//   --thread --test --debug --trace                          accepted (the CPU-side strategies
//                                                            they selected are retired)
//   --bvh         render through the acceleration structure (ESC_STAGE_BVH): what the flag was
//                 meant to do in the reference (main.cpp:566-570,792-800), same image as without;
//                 proven bounds only (triangle meshes go through the default path's lists / groups)
//   --bvh-tree    the tree for triangle meshes as well (ESC_RENDER_BVH_HEURISTIC_PADS)
//   --ispc        render through the `trace` drop-in symbol on flatten_scene_ispc-style arrays, in
//                 (geometry, face) order: the scalar path's image bit for bit.  NOT the reference's
//                 centroid-x sort (flatten_iscp.cpp:110) -- parity with the reference's own --ispc
//                 image is unpinned either way (its run is undefined before it reaches trace)
//   --ispc-sorted the same with that sort (the reference's primitive order: ties and, with two or
//                 more lights, first occluders follow it)
//   -w W,H        window size.  NOTE: in the reference this flag writes into `look`
//                 (main.cpp:515-529) and the window stays 1024x768; here
//                 it does what its help text says.
//   --gpus N      8-row strips over N bands from this one process; bands share the GPUs there are and
//                 their strips go straight to the host (esc_render_frame_multi)
//   --rccl        with --gpus: one GPU per band, strips gathered to device 0 over RCCL instead
//                 (opt-in: its exchange has not run on more than one device yet)
//   --scene c2|c3|c4|c5[:n]   synthetic BASELINE.json workload instead of -m
//   --shadows 0|1  --seed S  --face K   light-face choice: hashed (default) or fixed K
//   --dump-f32 path           raw fp32 RGB framebuffer, (h*W+w)*3 order, h = 0 bottom
//   --spp N       anti-aliased frame: N = n*n samples per pixel on a regular sub-pixel grid, n in 1..8
//                 (esc_render_supersampled; one GPU, not with --ispc or --bvh).  The frame is the mean
//                 of the samples; the PPM is written as usual
//   --adaptive T  with --spp: only the pixels that differ from a 4-neighbour by more than T (finite, >= 0) in
//                 some channel of the 1-sample frame get the N samples; the others keep the frame's value
//                 (esc_render_adaptive).  Not with --bounces
//   --bounces N   mirror reflections: up to N (0..16) specular bounces weighted by the materials' ks
//                 (esc_render_traced; combinable with --spp, otherwise under --spp's restrictions)
//   --bias X      with --bounces: a bounce starts X (finite, >= 0; default 1e-4) off its surface
//   --refract     with --bounces: materials with a transmission entry (MTL Tf / Ni under illum 4, 6, 7, 9)
//                 refract; total internal reflection reflects (esc_render_traced_ex, ESC_TRANSMIT_REFRACT)
//   --fresnel     with --bounces: the same, and Schlick's term picks reflection or refraction per
//                 sample by a hash (ESC_TRANSMIT_FRESNEL; use it with --spp).  Not with --refract
//   --ao K        ambient occlusion: the image the run would otherwise write is multiplied, pixel by pixel,
//                 by the share of K (1..64) hemisphere directions above the pixel centre's hit point that are
//                 open within --ao-radius (esc_render_ambient, esc_modulate; one GPU, not with --ispc)
//   --ao-radius R with --ao, required: how far a sample ray looks (finite, > 0)
//   --ao-sets S   with --ao: S (1..64, default 16) sets of K cosine-weighted directions, one drawn per pixel
//   --ao-bias B   with --ao: the sample rays start B (finite, >= 0; default 1e-4) off the surface
//   --ao-seed N   with --ao: seed of the direction table and of the per-pixel draw (default 0)
//   --denoise L   with --ao: the visibility (--skylight: the light) goes through L (1..8) iterations of the
//                 edge-stopping a-trous filter before it meets the image, guided by the frame's normals, hit
//                 positions and object ids (esc_render_gbuffer, esc_filter_guided)
//   --denoise-normal C  with --denoise: a neighbour counts when its normal has dot >= C with the pixel's
//                 (default 0.9)
//   --denoise-plane X   with --denoise: ... and it lies within X (>= 0) of the pixel's tangent plane (default
//                 --ao-radius / 4)
//   --temporal N  with --ao: N (1..64) frames are rendered and the visibility (--skylight: the light) is
//                 accumulated over them (esc_render_gbuffer, esc_temporal_accumulate).  Frame f = 0 .. N-1 has
//                 its eye at the view's (-v) minus --temporal-step times (N-1-f), per component in fp32, so the
//                 last frame is the given view; the look-at stays; the AO seed of frame f is f (not with --ao-seed).  The stops are
//                 --denoise-normal / --denoise-plane with --denoise's defaults; --denoise L filters the
//                 accumulated image of the last frame
//   --temporal-step x,y,z   with --temporal: how far the eye moves per frame (finite; default 0,0,0)
//   --temporal-max M   with --temporal: the history length saturates at M (1..65536, default 32)
//   --temporal-taps T  with --temporal: 1 = the nearest history pixel, 4 = bilinear (default)
//   --sky Z/H/G   environment: a vertical gradient (zenith, horizon, ground colours, each r,g,b; finite) that
//                 the rays which leave the scene see, primary rays and bounces alike (esc_environment_sky,
//                 esc_set_environment).  The frame is rendered through esc_render_traced_ex, at depth 0 when
//                 --bounces is absent (one GPU, not with --ispc, --bvh, --bvh-tree or --adaptive)
//   --sky-res N   with --sky: texels per side of the cube (1..1024, default 64)
//   --skylight    with --sky and --ao K --ao-radius R: the sky lights the scene.  Instead of being multiplied
//                 by the visibility, the image gains, pixel by pixel, kd times the mean of what the open ones
//                 of the K directions see of the sky (esc_render_skylight, esc_add_light; one GPU, not with
//                 --ispc)
//   --aperture A  with --spp N: depth of field.  Sample k of a pixel leaves lens point k of one of 16 sets of N
//                 points of a disk of radius A (finite, >= 0; scene units) about the eye and aims at the plane
//                 that stays sharp (esc_lens_disk_table, esc_set_lens_table, esc_render_lens).  Combines with
//                 --bounces, --refract, --fresnel and --sky; not with --adaptive, --ao, --ispc or --gpus
//   --focus D     with --aperture: the distance of the sharp plane along the view axis (finite, > 0; default
//                 the fp32 length of look-at minus view)
//   --lens-seed S with --aperture: seed of the lens table and of the per-pixel draw of a set (default 0)
//   --help        print the options and leave
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "esctp1_rt.h"

namespace {

[[noreturn]] void die(const std::string &msg) {
  std::cerr << "ESCViewer2021: " << msg << std::endl;
  std::exit(1);
}

void check(int rc, const char *what) {
  if (rc < 0) die(std::string(what) + ": " + esc_last_error());
}

// main.cpp:480-493: strtok on ',' + atof, exactly n components
void parse_floats(const char *flag, char *arg, float *out, int n, const char *err) {
  if (!arg) die(std::string(flag) + " needs a value");
  int i = 0;
  for (char *tok = std::strtok(arg, ","); tok; tok = std::strtok(nullptr, ",")) {
    if (i < n) out[i] = (float)std::atof(tok);
    i++;
  }
  if (i != n) die(err);
}

const char *kUsage =
    "ESCViewer2021 [-m model.obj | --scene c2|c3|c4|c5[:n]] [-o out.ppm] [-v x,y,z] [-l x,y,z] [-w W,H]\n"
    "  --thread --bvh --bvh-tree --ispc --ispc-sorted --test --debug --trace   the reference's modes\n"
    "  --gpus N [--rccl]          strips over N bands\n"
    "  --shadows 0|1 --seed S --face K   shadow rays, light-face choice\n"
    "  --dump-f32 path            raw fp32 framebuffer\n"
    "  --spp N                    N = n*n samples per pixel, n in 1..8\n"
    "  --adaptive T               with --spp: refine only pixels whose contrast to a 4-neighbour exceeds T\n"
    "  --bounces N                up to N (0..16) bounces: mirror reflections weighted by ks\n"
    "  --bias X                   with --bounces: a bounce starts X off its surface (default 1e-4)\n"
    "  --refract                  with --bounces: transmissive materials (Tf / Ni) refract\n"
    "  --fresnel                  with --bounces: Schlick's term picks reflection or refraction per sample\n"
    "  --ao K --ao-radius R       multiply the image by the visibility of K hemisphere directions within R\n"
    "  --ao-sets S --ao-bias B --ao-seed N   with --ao: direction sets (16), surface offset (1e-4), seed (0)\n"
    "  --denoise L                with --ao: L (1..8) passes of the edge-stopping filter over vis / light\n"
    "  --denoise-normal C --denoise-plane X   with --denoise: normal (0.9) and plane (--ao-radius / 4) stops\n"
    "  --temporal N               with --ao: accumulate vis / light over N (1..64) frames, frame f seeded with f;\n"
    "                             the stops are --denoise-normal / --denoise-plane, --denoise filters the result\n"
    "  --temporal-step x,y,z --temporal-max M --temporal-taps 1|4   with --temporal: the eye's move per frame\n"
    "                             (0,0,0; the last frame is the -v view), the longest history (32), taps (4)\n"
    "  --sky zr,zg,zb/hr,hg,hb/gr,gg,gb   rays that leave the scene see a zenith / horizon / ground gradient\n"
    "  --sky-res N                with --sky: texels per side of the environment cube (1..1024, default 64)\n"
    "  --skylight                 with --sky and --ao K --ao-radius R: add the sky's light on the open directions\n"
    "                             to the image instead of multiplying it by the visibility\n"
    "  --aperture A               with --spp: depth of field through a lens of radius A (scene units)\n"
    "  --focus D --lens-seed S    with --aperture: the sharp plane's distance (|look - eye|), the lens seed (0)\n"
    "  --help                     this text\n";

// --ao's values: a whole number in [lo, hi], or a finite float (> 0, or >= 0), with nothing after it
long parse_whole(const char *flag, const char *next, long lo, long hi) {
  if (!next) die(std::string(flag) + " needs a value");
  char *end = nullptr;
  const long v = std::strtol(next, &end, 10);
  if (end == next || *end != '\0' || v < lo || v > hi)
    die(std::string(flag) + " must be a whole number from " + std::to_string(lo) + " to " + std::to_string(hi) +
        ", got " + next);
  return v;
}

float parse_finite(const char *flag, const char *next, bool zero_ok) {
  if (!next) die(std::string(flag) + " needs a value");
  char *end = nullptr;
  const float v = std::strtof(next, &end);
  if (end == next || *end != '\0' || !std::isfinite(v) || !(zero_ok ? v >= 0.f : v > 0.f))
    die(std::string(flag) + " must be a finite number " + (zero_ok ? ">= 0" : "> 0") + ", got " + next);
  return v;
}

// --sky's value: three colours separated by '/', each three finite numbers separated by ','
void parse_sky(const char *next, float out[9]) {
  const std::string err = "--sky needs zr,zg,zb/hr,hg,hb/gr,gg,gb with nine finite numbers";
  if (!next) die(err);
  const char *p = next;
  for (int k = 0; k < 9; ++k) {
    char *end = nullptr;
    const float v = std::strtof(p, &end);
    if (end == p || !std::isfinite(v)) die(err + ", got " + next);
    out[k] = v;
    const char want = k == 8 ? '\0' : (k % 3 == 2 ? '/' : ',');
    if (*end != want) die(err + ", got " + next);
    p = end + 1;
  }
}

// --temporal-step's value: three finite numbers separated by ','
void parse_step(const char *next, float out[3]) {
  const std::string err = "--temporal-step needs x,y,z with three finite numbers";
  if (!next) die(err);
  const char *p = next;
  for (int k = 0; k < 3; ++k) {
    char *end = nullptr;
    const float v = std::strtof(p, &end);
    if (end == p || !std::isfinite(v) || *end != (k == 2 ? '\0' : ',')) die(err + ", got " + next);
    out[k] = v;
    p = end + 1;
  }
}

} // namespace

int main(int argc, char *argv[]) {
  std::string modelname, outputname, dumpname, synthetic;
  bool threaded = false, flat = false, ispc = false, use_rccl = false, ispc_sorted = false, bvh_tree = false;
  int debug = 1; // INFO, debug.h:3
  float eye[3] = {0, 1, 3}, look[3] = {0, 1, 0}; // main.cpp:426
  int W = 1024, H = 768;                         // main.cpp:427
  int gpus = 1, shadows = 1, fixed_face = -1, spp = 0, bounces = -1;
  float bias = 1e-4f, adaptive = 0.f;
  bool have_adaptive = false;
  bool have_bias = false, refract = false, fresnel = false;
  unsigned long long seed = 0;
  int ao = 0, ao_sets = 16;
  float ao_radius = 0.f, ao_bias = 1e-4f;
  unsigned long long ao_seed = 0;
  bool have_ao_radius = false, have_ao_extra = false;
  bool sky = false, have_sky_res = false, skylight = false;
  int denoise = 0;
  float denoise_normal = 0.9f, denoise_plane = 0.f;
  bool have_denoise_extra = false, have_denoise_plane = false;
  int temporal = 0, temporal_max = 32, temporal_taps = 4;
  float temporal_step[3] = {0.f, 0.f, 0.f};
  bool have_temporal_extra = false, have_ao_seed = false;
  float sky_colours[9] = {0};
  int sky_res = 64;
  float aperture = 0.f, focus = 0.f;
  unsigned long long lens_seed = 0;
  bool have_aperture = false, have_focus = false, have_lens_seed = false;

  for (int arg = 1; arg < argc; arg++) {
    const std::string a = argv[arg];
    char *next = (arg + 1 < argc) ? argv[arg + 1] : nullptr;
    if (a == "--thread") { threaded = true; continue; }
    if (a == "--bvh") { flat = true; continue; }
    if (a == "--ispc") { ispc = true; continue; }
    if (a == "--test") { continue; }
    if (a == "--debug") { debug = 2; continue; }
    if (a == "--trace") { debug = 3; continue; }
    if (a == "-m") { if (!next) die("-m needs a path"); modelname = next; arg++; continue; }
    if (a == "-o") { if (!next) die("-o needs a path"); outputname = next; arg++; continue; }
    if (a == "-v") { parse_floats("-v", next, eye, 3, "Error parsing view"); arg++; continue; }
    if (a == "-l") { parse_floats("-l", next, look, 3, "Error parsing look"); arg++; continue; }
    if (a == "-w") {
      float wh[2];
      parse_floats("-w", next, wh, 2, "Error parsing window size");
      W = (int)wh[0];
      H = (int)wh[1];
      arg++;
      continue;
    }
    if (a == "--gpus") { if (!next) die("--gpus needs N"); gpus = std::atoi(next); arg++; continue; }
    if (a == "--bvh-tree") { flat = bvh_tree = true; continue; }
    if (a == "--rccl") { use_rccl = true; continue; }
    if (a == "--no-rccl") { use_rccl = false; continue; } // (the default; kept for old command lines)
    if (a == "--ispc-sorted") { ispc = ispc_sorted = true; continue; }
    if (a == "--scene") { if (!next) die("--scene needs a config"); synthetic = next; arg++; continue; }
    if (a == "--shadows") { if (!next) die("--shadows needs 0|1"); shadows = std::atoi(next); arg++; continue; }
    if (a == "--seed") { if (!next) die("--seed needs S"); seed = std::strtoull(next, nullptr, 0); arg++; continue; }
    if (a == "--face") { if (!next) die("--face needs K"); fixed_face = std::atoi(next); arg++; continue; }
    if (a == "--spp") {
      if (!next) die("--spp needs N");
      char *end = nullptr;
      const long v = std::strtol(next, &end, 10);
      int root = 0;
      for (int k = 1; k <= 8; k++)
        if (k * k == v) root = k;
      if (end == next || *end != '\0' || root == 0)
        die(std::string("--spp must be a square number from 1 to 64 (1, 4, 9, ..., 64), got ") + next);
      spp = (int)v;
      arg++;
      continue;
    }
    if (a == "--adaptive") {
      if (!next) die("--adaptive needs T");
      char *end = nullptr;
      const float v = std::strtof(next, &end);
      if (end == next || *end != '\0' || !(v >= 0.f) || !std::isfinite(v))
        die(std::string("--adaptive must be a finite number >= 0, got ") + next);
      adaptive = v;
      have_adaptive = true;
      arg++;
      continue;
    }
    if (a == "--bounces") {
      if (!next) die("--bounces needs N");
      char *end = nullptr;
      const long v = std::strtol(next, &end, 10);
      if (end == next || *end != '\0' || v < 0 || v > ESC_TRACE_MAX_DEPTH)
        die(std::string("--bounces must be a whole number from 0 to 16, got ") + next);
      bounces = (int)v;
      arg++;
      continue;
    }
    if (a == "--bias") {
      if (!next) die("--bias needs X");
      char *end = nullptr;
      const float v = std::strtof(next, &end);
      if (end == next || *end != '\0' || !(v >= 0.f) || !std::isfinite(v))
        die(std::string("--bias must be a finite number >= 0, got ") + next);
      bias = v;
      have_bias = true;
      arg++;
      continue;
    }
    if (a == "--refract") { refract = true; continue; }
    if (a == "--fresnel") { fresnel = true; continue; }
    if (a == "--ao") { ao = (int)parse_whole("--ao", next, 1, 64); arg++; continue; }
    if (a == "--ao-radius") {
      ao_radius = parse_finite("--ao-radius", next, false);
      have_ao_radius = true;
      arg++;
      continue;
    }
    if (a == "--ao-sets") {
      ao_sets = (int)parse_whole("--ao-sets", next, 1, 64);
      have_ao_extra = true;
      arg++;
      continue;
    }
    if (a == "--ao-bias") {
      ao_bias = parse_finite("--ao-bias", next, true);
      have_ao_extra = true;
      arg++;
      continue;
    }
    if (a == "--ao-seed") {
      if (!next) die("--ao-seed needs N");
      char *end = nullptr;
      ao_seed = std::strtoull(next, &end, 0);
      if (end == next || *end != '\0') die(std::string("--ao-seed must be a whole number, got ") + next);
      have_ao_extra = have_ao_seed = true;
      arg++;
      continue;
    }
    if (a == "--temporal") { temporal = (int)parse_whole("--temporal", next, 1, 64); arg++; continue; }
    if (a == "--temporal-step") {
      parse_step(next, temporal_step);
      have_temporal_extra = true;
      arg++;
      continue;
    }
    if (a == "--temporal-max") {
      temporal_max = (int)parse_whole("--temporal-max", next, 1, 65536);
      have_temporal_extra = true;
      arg++;
      continue;
    }
    if (a == "--temporal-taps") {
      if (!next) die("--temporal-taps needs a value");
      if (std::strcmp(next, "1") != 0 && std::strcmp(next, "4") != 0)
        die(std::string("--temporal-taps must be 1 or 4, got ") + next);
      temporal_taps = next[0] - '0';
      have_temporal_extra = true;
      arg++;
      continue;
    }
    if (a == "--denoise") { denoise = (int)parse_whole("--denoise", next, 1, 8); arg++; continue; }
    if (a == "--denoise-normal") {
      if (!next) die("--denoise-normal needs a value");
      char *end = nullptr;
      denoise_normal = std::strtof(next, &end);
      if (end == next || *end != '\0' || !std::isfinite(denoise_normal))
        die(std::string("--denoise-normal must be a finite number, got ") + next);
      have_denoise_extra = true;
      arg++;
      continue;
    }
    if (a == "--denoise-plane") {
      denoise_plane = parse_finite("--denoise-plane", next, true);
      have_denoise_extra = have_denoise_plane = true;
      arg++;
      continue;
    }
    if (a == "--sky") { parse_sky(next, sky_colours); sky = true; arg++; continue; }
    if (a == "--sky-res") {
      sky_res = (int)parse_whole("--sky-res", next, 1, ESC_ENV_MAX_RES);
      have_sky_res = true;
      arg++;
      continue;
    }
    if (a == "--skylight") { skylight = true; continue; }
    if (a == "--aperture") {
      aperture = parse_finite("--aperture", next, true);
      have_aperture = true;
      arg++;
      continue;
    }
    if (a == "--focus") {
      focus = parse_finite("--focus", next, false);
      have_focus = true;
      arg++;
      continue;
    }
    if (a == "--lens-seed") {
      if (!next) die("--lens-seed needs S");
      char *end = nullptr;
      lens_seed = std::strtoull(next, &end, 0);
      if (end == next || *end != '\0') die(std::string("--lens-seed must be a whole number, got ") + next);
      have_lens_seed = true;
      arg++;
      continue;
    }
    if (a == "--help") {
      std::cout << kUsage;
      return 0;
    }
    if (a == "--dump-f32") { if (!next) die("--dump-f32 needs a path"); dumpname = next; arg++; continue; }
    die("Invalid Argument: " + a); // main.cpp:531-534
  }
  if (W < 2 || H < 2) die("window must be at least 2x2");
  if (gpus < 1) die("--gpus must be >= 1");
  if (spp && (ispc || flat || gpus != 1)) die("--spp renders on one GPU and not with --ispc, --bvh or --bvh-tree");
  if (bounces >= 0 && (ispc || flat || gpus != 1))
    die("--bounces renders on one GPU and not with --ispc, --bvh or --bvh-tree");
  if (have_adaptive && !spp) die("--adaptive needs --spp");
  if (have_adaptive && bounces >= 0) die("--adaptive refines plain frames: not with --bounces");
  if (have_bias && bounces < 0) die("--bias needs --bounces");
  if (refract && fresnel) die("--refract and --fresnel exclude each other");
  if (refract && bounces < 0) die("--refract needs --bounces");
  if (fresnel && bounces < 0) die("--fresnel needs --bounces");
  if (skylight && (ispc || gpus != 1)) die("--skylight renders on one GPU and not with --ispc");
  if (skylight && !sky) die("--skylight needs --sky");
  if (skylight && (!ao || !have_ao_radius)) die("--skylight needs --ao K --ao-radius R");
  if (ao && !have_ao_radius) die("--ao needs --ao-radius");
  if (!ao && (have_ao_radius || have_ao_extra)) die("--ao-radius, --ao-sets, --ao-bias and --ao-seed need --ao");
  if (ao && (ispc || gpus != 1)) die("--ao renders on one GPU and not with --ispc");
  if (denoise && !ao) die("--denoise needs --ao");
  if (temporal && !ao) die("--temporal needs --ao");
  if (!temporal && have_temporal_extra) die("--temporal-step, --temporal-max and --temporal-taps need --temporal");
  if (temporal && have_ao_seed) die("--temporal seeds frame f with f: not with --ao-seed");
  if (!denoise && !temporal && have_denoise_extra) die("--denoise-normal and --denoise-plane need --denoise");
  if (have_sky_res && !sky) die("--sky-res needs --sky");
  if (sky && (ispc || flat || gpus != 1)) die("--sky renders on one GPU and not with --ispc, --bvh or --bvh-tree");
  if (sky && have_adaptive) die("--sky is seen by traced frames: not with --adaptive");
  if (have_aperture && !spp) die("--aperture needs --spp");
  if (have_aperture && (have_adaptive || ao)) die("--aperture renders traced frames: not with --adaptive or --ao");
  if (!have_aperture && (have_focus || have_lens_seed)) die("--focus and --lens-seed need --aperture");

  esc_scene *scene = esc_scene_new();
  if (!scene) die("out of memory");
  if (!synthetic.empty()) {
    int n = 0;
    std::string cfg = synthetic;
    const size_t colon = cfg.find(':');
    if (colon != std::string::npos) {
      n = std::atoi(cfg.c_str() + colon + 1);
      cfg = cfg.substr(0, colon);
    }
    check(esc_scene_synthetic(scene, cfg.c_str(), n), "synthetic scene");
    if (modelname.empty()) esc_synthetic_view(eye, look);
  }
  if (!modelname.empty()) check(esc_scene_load_obj(scene, modelname.c_str()), "loadobj"); // main.cpp:540-543

  const float aspect = float(W) / H; // main.cpp:548
  const float vfov = 60.f;           // main.cpp:549
  const float vup[3] = {0, 1, 0};    // main.cpp:550
  esc_camera cam;
  esc_camera_init(&cam, eye, look, vup, vfov, aspect);

  std::vector<float> image((size_t)W * H * 3, 0.f);
  esc_render_options opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.shadows = shadows;
  opts.face_mode = fixed_face >= 0 ? ESC_FACE_FIXED : ESC_FACE_HASH;
  opts.fixed_face = fixed_face >= 0 ? fixed_face : 0;
  opts.seed = seed;
  if (flat) opts.stage = ESC_STAGE_BVH; // tree build happens inside the timed region, like the
                                        // reference's buildBVH sits before its render clock
  if (bvh_tree) opts.flags |= ESC_RENDER_BVH_HEURISTIC_PADS;
  opts.flags |= ESC_RENDER_NO_COUNTERS; // the viewer prints no ray statistics: no instrumentation in its frames

  // Device set-up is to this program what dynamic linking is to the reference: it happens before
  // the clock.  One device: context, scene tables in HBM and the kernels' code object (a 2x2
  // frame makes the runtime load it) are ready when the clock starts; what is timed is the
  // frame itself and its copy back to the host, like the row loop of main.cpp:583-645.
  esc_context *ctx = nullptr;
  if (!ispc && gpus == 1) {
    check(esc_context_create(0, &ctx), "context");
    check(esc_upload_scene(ctx, scene), "upload");
    float tiny[2 * 2 * 3];
    esc_render_options w = opts;
    w.stage = ESC_STAGE_AUTO;
    check(esc_render_frame_host(ctx, &cam, 2, 2, &w, tiny, nullptr), "warm-up");
  } else if (ispc) { // the seam owns its context: a 2x2 call through it does the same
    esc_flat_scene *fs = nullptr;
    check(esc_flatten_ispc(scene, 0, &fs), "flatten_scene_ispc");
    ispc_cam icam;
    esc_new_ispc_cam(&icam, eye, look, vup, vfov, aspect);
    int32_t nt = 0, nl = 0, nlt = 0;
    ispc_triangle *tris = esc_flat_triangles(fs, &nt);
    ispc_light *lights = esc_flat_lights(fs, &nl);
    ispc_triangle *ltris = esc_flat_light_triangles(fs, &nlt);
    float tiny[2 * 2 * 3];
    trace(2, 2, &icam, nt, tris, nl, lights, nlt, ltris, tiny, 0, 0);
    esc_flat_free(fs);
  }

  // start the clock! (main.cpp:583)
  auto start_time = std::chrono::high_resolution_clock::now();
  if (ispc) {
    // main.cpp:591-624: flatten inside the timed region, then the exported trace symbol
    esc_flat_scene *fs = nullptr;
    // (geometry, face) order, NOT the reference's centroid-x sort (flatten_iscp.cpp:110): the
    // sort permutes primitive indices, which changes equal-t ties and -- with two or more lights
    // -- the first occluder occlusion() reports in index order, whose t2 the next light's shadow
    // ray starts from (quirk S3).  Unsorted, --ispc writes the scalar path's image bit for bit.
    // --ispc-sorted keeps the reference's sort: its primitive order, hence its ties and first
    // occluders; no reference fixture pins that image (the reference's own --ispc run is undefined
    // behaviour before it reaches trace), so it is "parity unpinned".
    check(esc_flatten_ispc(scene, /*sort_by_centroid_x=*/ispc_sorted ? 1 : 0, &fs), "flatten_scene_ispc");
    ispc_cam icam;
    esc_new_ispc_cam(&icam, eye, look, vup, vfov, aspect);
    int32_t nt = 0, nl = 0, nlt = 0;
    ispc_triangle *tris = esc_flat_triangles(fs, &nt);
    ispc_light *lights = esc_flat_lights(fs, &nl);
    ispc_triangle *ltris = esc_flat_light_triangles(fs, &nlt);
    if (debug >= 2)
      std::cout << "Before trace: \n num_flat_triangles   = " << nt << "\n num_lights      = " << nl
                << "\n num_light_faces = " << nlt << std::endl;
    trace(W, H, &icam, nt, tris, nl, lights, nlt, ltris, image.data(), debug, 0);
    esc_flat_free(fs);
  } else if (ctx && (spp || bounces >= 0 || sky)) {
    // device framebuffer of esc_render_supersampled / esc_render_traced, copied back like
    // esc_render_frame_host's
    esc_render_options so = opts;
    so.flags = 0;
    float *d_image = nullptr;
    if (hipMalloc((void **)&d_image, image.size() * sizeof(float)) != hipSuccess) die("out of device memory");
    if (sky) {
      std::vector<float> cube((size_t)6 * sky_res * sky_res * 3);
      check(esc_environment_sky(sky_res, sky_colours, sky_colours + 3, sky_colours + 6, cube.data()), "sky");
      check(esc_set_environment(ctx, sky_res, cube.data()), "sky");
    }
    if (have_aperture) {
      // 16 sets of spp lens points, one set per pixel; sample k of a pixel goes through lens point k
      const int lens_sets = 16;
      std::vector<float> table((size_t)lens_sets * spp * 2);
      check(esc_lens_disk_table(lens_sets, spp, lens_seed, table.data()), "lens table");
      check(esc_set_lens_table(ctx, lens_sets, spp, table.data()), "lens table");
      if (!have_focus) { // the look-at point stays sharp
        const float v[3] = {look[0] - eye[0], look[1] - eye[1], look[2] - eye[2]};
        focus = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        if (!(focus > 0.f) || !std::isfinite(focus)) die("--aperture: the view and the look-at point coincide; give --focus");
      }
      const esc_trace_options to = {bounces >= 0 ? bounces : 0, bias,
                                    refract ? ESC_TRANSMIT_REFRACT : fresnel ? ESC_TRANSMIT_FRESNEL : ESC_TRANSMIT_OFF,
                                    0};
      const esc_lens_options lo = {aperture, focus, lens_seed, {0, 0}};
      check(esc_render_lens(ctx, &cam, W, H, spp, &so, &to, &lo, d_image, nullptr), "render");
    } else if (sky) {
      const esc_trace_options to = {bounces >= 0 ? bounces : 0, bias,
                                    refract ? ESC_TRANSMIT_REFRACT : fresnel ? ESC_TRANSMIT_FRESNEL : ESC_TRANSMIT_OFF,
                                    0};
      check(esc_render_traced_ex(ctx, &cam, W, H, spp ? spp : 1, &so, &to, d_image, nullptr), "render");
    } else if (bounces >= 0 && (refract || fresnel)) {
      const esc_trace_options to = {bounces, bias, refract ? ESC_TRANSMIT_REFRACT : ESC_TRANSMIT_FRESNEL, 0};
      check(esc_render_traced_ex(ctx, &cam, W, H, spp ? spp : 1, &so, &to, d_image, nullptr), "render");
    } else if (bounces >= 0)
      check(esc_render_traced(ctx, &cam, W, H, spp ? spp : 1, bounces, bias, &so, d_image, nullptr), "render");
    else if (have_adaptive) {
      const esc_adaptive_options ao = {spp, adaptive, 0, 0};
      check(esc_render_adaptive(ctx, &cam, W, H, &so, &ao, d_image, nullptr, nullptr), "render");
    } else
      check(esc_render_supersampled(ctx, &cam, W, H, spp, &so, d_image, nullptr), "render");
    check(esc_context_synchronize(ctx), "render");
    if (hipMemcpy(image.data(), d_image, image.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      die("copy back failed");
    (void)hipFree(d_image);
  } else if (ctx) {
    check(esc_render_frame_host(ctx, &cam, W, H, &opts, image.data(), nullptr), "render");
  } else {
    // N devices from this one process.  Default: the band-sharing path that copies every band's
    // strips straight to the host (esc_render_frame_multi; runs with any number of GPUs, verified on
    // the GPU box).  --rccl: a GPU per band, strips gathered to device 0 over RCCL
    // (esc_render_frame_multi_rccl) -- opt-in, because its n > 1 exchange (grouped ncclSend /
    // ncclRecv) has not run on more than one device yet.
    std::vector<float> ms((size_t)gpus, 0.f);
    int rc = ESC_ERR_RCCL;
    if (use_rccl && esc_rccl_available())
      rc = esc_render_frame_multi_rccl(scene, &cam, W, H, &opts, gpus, image.data(), nullptr,
                                       ms.data());
    if (rc != ESC_OK) {
      if (use_rccl) std::cerr << " RCCL path not used: " << esc_last_error() << std::endl;
      check(esc_render_frame_multi(scene, &cam, W, H, &opts, gpus, image.data(), nullptr, ms.data()),
            "render");
    }
    if (debug >= 2)
      for (int i = 0; i < gpus; i++) std::cerr << " band " << i << " kernel ms: " << ms[i] << std::endl;
  }
  if (ao) {
    // the frame back on the device, the pixel centres' visibility (--skylight: the sky's light on them), the
    // product (the sum) in place, and home again
    const size_t n = (size_t)W * H, ch = skylight ? 3 : 1;
    float *d_image = nullptr, *d_vis = nullptr; // d_vis: W*H visibilities, or with --skylight W*H*3 of light
    if (hipMalloc((void **)&d_image, image.size() * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&d_vis, n * ch * sizeof(float)) != hipSuccess)
      die("out of device memory");
    if (hipMemcpy(d_image, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      die("copy to the device failed");
    // --denoise, --temporal: a frame's guides (normal, position | geom, prim); --temporal keeps the previous
    // frame's too, and alternates the accumulated image and the history lengths between two buffers each
    float *d_guides[2] = {nullptr, nullptr}, *d_acc[2] = {nullptr, nullptr}, *d_filtered = nullptr;
    int32_t *d_n[2] = {nullptr, nullptr};
    for (int k = 0; k < (temporal ? 2 : denoise ? 1 : 0); ++k)
      if (hipMalloc((void **)&d_guides[k], n * 8 * sizeof(float)) != hipSuccess) die("out of device memory");
    if (temporal) {
      for (int k = 0; k < 2; ++k)
        if (hipMalloc((void **)&d_acc[k], n * ch * sizeof(float)) != hipSuccess ||
            hipMalloc((void **)&d_n[k], n * sizeof(int32_t)) != hipSuccess)
          die("out of device memory");
      // the first frame's history: no length anywhere
      if (hipMemset(d_acc[0], 0, n * ch * sizeof(float)) != hipSuccess ||
          hipMemset(d_n[0], 0, n * sizeof(int32_t)) != hipSuccess)
        die("clearing the history failed");
    }
    const float stop_plane = have_denoise_plane ? denoise_plane : ao_radius / 4.f;
    const auto guides_of = [n](float *g) {
      int32_t *geom = reinterpret_cast<int32_t *>(g + 6 * n);
      return esc_guides{g, g + 3 * n, geom, geom + n};
    };
    const float *d_use = d_vis;
    esc_camera prev_cam = cam;
    const int frames = temporal ? temporal : 1;
    for (int f = 0; f < frames; ++f) {
      esc_camera fcam = cam;
      unsigned long long fseed = ao_seed;
      if (temporal) { // the eye of frame f; the last frame is the given view
        float feye[3];
        for (int k = 0; k < 3; ++k) feye[k] = eye[k] - temporal_step[k] * float(frames - 1 - f);
        esc_camera_init(&fcam, feye, look, vup, vfov, aspect);
        fseed = (unsigned long long)f;
      }
      std::vector<float> table((size_t)ao_sets * ao * 3);
      check(esc_ambient_cosine_table(ao_sets, ao, fseed, table.data()), "ambient table");
      check(esc_set_ambient_table(ctx, ao_sets, ao, table.data()), "ambient table");
      const esc_ambient_options ao_opts = {ao, ao_sets, ao_radius, ao_bias, fseed, 0u, 0u};
      if (skylight) check(esc_render_skylight(ctx, &fcam, W, H, &ao_opts, nullptr, d_vis, nullptr, nullptr), "skylight");
      else check(esc_render_ambient(ctx, &fcam, W, H, &ao_opts, d_vis, nullptr), "ambient");
      float *g = d_guides[f & 1];
      if (g) {
        const esc_guides gs = guides_of(g);
        check(esc_render_gbuffer(ctx, &fcam, W, H, 0u, g, g + 3 * n, nullptr, nullptr,
                                 const_cast<int32_t *>(gs.geom), const_cast<int32_t *>(gs.prim)), "gbuffer");
      }
      if (temporal) {
        const esc_guides cur = guides_of(g), prev = f ? guides_of(d_guides[(f & 1) ^ 1]) : cur;
        const esc_camera pc = f ? prev_cam : fcam;
        const esc_temporal_options t_opts = {temporal_taps, temporal_max, denoise_normal, stop_plane, 1, {0, 0, 0}};
        check(esc_temporal_accumulate(ctx, &pc, W, H, (int32_t)ch, d_vis, &cur, d_acc[f & 1], d_n[f & 1], &prev,
                                      &t_opts, d_acc[(f & 1) ^ 1], d_n[(f & 1) ^ 1]), "temporal");
        d_use = d_acc[(f & 1) ^ 1];
        prev_cam = fcam;
      }
    }
    if (denoise) {
      // --denoise: the filter on vis / light, or on what --temporal accumulated, under the last frame's guides
      if (hipMalloc((void **)&d_filtered, n * ch * sizeof(float)) != hipSuccess) die("out of device memory");
      const esc_guides gs = guides_of(d_guides[(frames - 1) & 1]);
      const esc_filter_options f_opts = {denoise, denoise_normal, stop_plane, 1, {0, 0}};
      check(esc_filter_guided(ctx, W, H, (int32_t)ch, d_use, gs.normal, gs.position, gs.geom, gs.prim, &f_opts,
                              d_filtered), "denoise");
      d_use = d_filtered;
    }
    if (skylight) check(esc_add_light(ctx, (int64_t)W * H, d_image, d_use, d_image, nullptr), "add light");
    else check(esc_modulate(ctx, (int64_t)W * H, d_image, d_use, d_image, nullptr), "modulate");
    check(esc_context_synchronize(ctx), "ambient");
    for (int k = 0; k < 2; ++k) {
      (void)hipFree(d_guides[k]);
      (void)hipFree(d_acc[k]);
      (void)hipFree(d_n[k]);
    }
    (void)hipFree(d_filtered);
    if (hipMemcpy(image.data(), d_image, image.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      die("copy back failed");
    (void)hipFree(d_image);
    (void)hipFree(d_vis);
  }
  auto end_time = std::chrono::high_resolution_clock::now();

  // main.cpp:647-654
  std::cerr << "\n Threaded  : " << std::boolalpha << threaded << std::endl;
  std::cerr << " Flattened : " << std::boolalpha << flat << std::endl;
  std::cerr << " ISPC      : " << std::boolalpha << ispc << std::endl;
  std::cerr << "\n Duration  : "
            << std::chrono::duration_cast<std::chrono::milliseconds>(end_time - start_time).count()
            << std::endl;

  if (!dumpname.empty()) {
    std::ofstream f(dumpname, std::ios::binary);
    f.write(reinterpret_cast<const char *>(image.data()), (std::streamsize)(image.size() * 4));
    if (!f) die("cannot write " + dumpname);
  }
  if (!outputname.empty()) { // main.cpp:658-691
    check(esc_write_ppm(outputname.c_str(), image.data(), W, H), "write ppm");
    std::cout << "Rendered image in: " << outputname << std::endl;
  } else {
    std::cout << "Nothing saved: use -o to save rendered image" << std::endl;
  }
  if (ctx) esc_context_destroy(ctx);
  esc_scene_free(scene);
  return 0;
}
