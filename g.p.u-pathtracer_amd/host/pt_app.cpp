// pt_app.cpp — headless "App render loop": what BasicScene::run() (GpuPathTracer/
// BasicScene.cpp:368-477) does per frame, minus window/GL/ImGui, over the C ABI.
//
//   per frame:  sync (BasicScene.cpp:395) → frame seed (:397) → constantPdf logic (:399)
//               → launchKernel (:404) → [display copy :424-432 → here: optional download]
//
// Usage: pt_app --mesh assets/cornell.ptmesh [--width 1280 --height 720 --frames 16 --spp 1
//               --depth 4 --mat 0..3 --no-spheres --no-materials --bk r g b --device 0
//               --out image.ppm|.png|.pfm  --checkpoint state.ckpt [--checkpoint-every N]
//               --resume state.ckpt --device-build --fix-estimators --nee --mis --gpus N --tile ROWS
//               --denoise-out image.ppm|.png|.pfm  --denoise-variance  --variance-out file.pfm  --until-error E --max-frames M
//               --pan-deg D --dolly S --spin-deg D --temporal-out image.ppm|.png|.pfm  --equirect
//               --env file.pfm [--env-scale S] [--env-nearest] [--env-light]
//               --camera pinhole|thinlens|ortho|fisheye|equirect [--aperture R --focus D --ortho-height S --fisheye-deg A] [--camera-loop]
//               --adaptive E --min-spp A --max-spp B [--pass-spp K] [--samples-out counts.pfm]
//               --tonemap clamp|reinhard|aces --transfer linear|srgb|gamma22 --exposure E|auto --white W]
// --gpus N splits the framebuffer over N contexts, one per GPU (devices device, device+1, ... modulo the number
// present, so N > 1 also runs on a one-GPU box): stripes of --tile rows (default 8) are dealt round-robin
// (pt_params.part_*), every context holds the whole scene and renders only its stripes of every frame — the random
// streams are keyed by the global pixel, so the merged image equals the one-GPU image bit for bit — and the stripes
// are gathered on the host when an image or a checkpoint is written (the reference is single-GPU).
// --device-build builds the BVH on the GPU (pt_build_bvh) instead of the host SAH/SBVH builder;
// --fix-estimators sets the PT_FLAG_* corrected-estimator switches (face-forward, cosine DIFF,
// glass fix, Russian roulette).
// --frames counts samples per pixel in total; --spp of them are folded per pt_render call.
// A mesh that carries materials (OBJ usemtl + .mtl, PTMESH2) is shaded with them
// (pt_upload_tri_materials) unless --no-materials.  --resume continues a checkpointed
// progressive render: the result is bit-identical to one uninterrupted run.
// --tonemap clamp|reinhard|aces, --transfer linear|srgb|gamma22, --exposure E|auto and --white W (reinhard: the scaled luminance shown
// as white) switch the display stage on: with any of them the .png / .ppm of --out, --denoise-out and --temporal-out are pt_tonemap's
// display words of the device buffer (the accumulator, the filtered frame, the history) — under --exposure auto after pt_meter, so the
// exposure never reaches the host — on every route, --camera, --equirect and --adaptive included; those three then accumulate as they
// do for a .pfm (PT_RAYS_HDR: the curve clamps, not the running mean).  Defaults: clamp, linear, 1.  A .pfm stays the linear floats.
// Without these flags every output byte is what it was.
// --denoise-out also writes the final accumulator through pt_denoise (guides from pt_render_aux, the library's default
// filter settings), format by extension as --out; with --gpus N the gathered frame is denoised on the first context.
// --denoise-variance makes --denoise-out run pt_denoise_variance instead: the run renders through pt_render_moments (as
// --variance-out does, --out unchanged) and the filter takes those moments with samples_per_frame = the samples per pixel behind
// the accumulator and no lengths.  Refused without --denoise-out, with --temporal-out and with --resume.
// --out is written first and is the same image with or without it.
// --variance-out and --until-error render through pt_render_moments: every context keeps the luminance moments of its stripes
// beside its accumulator (gathered with it).  --variance-out writes the variance of the pixel's mean luminance,
// max(0, m2 - m1^2) / (n - 1), as a PFM (one value per pixel, grey in three channels).  --until-error E keeps rendering calls of
// --spp samples past --frames (now the minimum) until pt_frame_error's mean_rse <= E, checked after every call, and never past
// --max-frames samples per pixel (required with it); it prints the samples rendered and the final figure.  With --gpus N the
// figure is computed on the first context from the gathered moments.  The --out image of such a run equals that of a plain run
// with the same number of samples byte for byte.  Checkpoints hold no moments, so neither option combines with --resume.
// --pan-deg D / --dolly S move the camera after every displayed frame (one pt_render call of --spp samples): front and right turn
// by D degrees about up, pos moves S along front.  A camera that moves restarts the accumulation, as the reference does when its
// camera is dirty: every displayed frame starts at sample_index = 1 and --out is the last frame alone.  --temporal-out runs the
// loop of a host with temporal accumulation (gpu_pathtracer_amd.TemporalHistory.push) after every displayed frame — pt_render_aux
// for the frame's camera, pt_temporal against the history of the frames before it, swap — and writes the history after the last
// frame, format by extension as --out; --denoise-out then filters the history instead of the last frame.  While the camera
// stands still the accumulator already is the mean of every sample from that viewpoint, so it enters the history once, after the
// last call, and --out is what it is without the flag, byte for byte.  --temporal-out works on one context over the whole frame
// and keeps no state a checkpoint could hold: it is refused with --gpus > 1, --resume, --checkpoint, --variance-out and
// --until-error; so are the motion options with --resume, --checkpoint and --until-error (nothing accumulates across frames).
// --spin-deg D moves the geometry instead: after every displayed frame the mesh (not the spheres) is turned to k x D degrees about
// (0, 1, 0) through the centre of its rest-pose bounds — on the host, in double, from the rest pose, so nothing drifts — uploaded to
// one of two device vertex buffers and applied with pt_refit_bvh (on every context of --gpus N).  Like a moving camera it restarts
// the accumulation every frame and is refused in the same combinations; with --temporal-out the history goes through
// pt_temporal_motion (ids from pt_render_aux, the previous and the current vertex buffer), which follows the turning triangles.
// D = 0 issues no refit and changes nothing: the output is byte-identical to a run without the option.
// --equirect renders a 360 x 180 degree latitude-longitude image seen from the camera position instead of the pinhole frame: column x
// looks at longitude (x - W/2) 2 pi / W from `front` towards `right`, row y at latitude (y - H/2) pi / H towards `up` (the pole), so
// the centre pixel looks along `front` and column 0 meets column W-1 behind it.  The rays are made on the host, one per pixel, and
// every call renders them through pt_render_rays (pixel y W + x draws the random numbers of that pixel of a pinhole frame):
// clamped mode when --out is a .png / .ppm, HDR when it is a .pfm.  There is no pinhole frame, so --equirect is refused with
// --denoise-out, --temporal-out, --variance-out, --until-error, --gpus > 1, --checkpoint, --resume and the motion options.
// --camera MODEL renders through one of the camera models of pt_camera_rays instead of pt_render's pinhole: one pt_render_camera
// call per --spp group makes every sample's jittered ray in the path kernel, so every sample has its own sub-pixel jitter and, for
// thinlens, its own point on the lens: anti-aliasing and depth of field.  --camera-loop renders the same samples the way the call
// is defined: per sample one pt_camera_rays call writes the jittered rays of every pixel for that sample's frame number on the
// device and one one-sample pt_render_rays call traces them (the loop of gpu_pathtracer_amd.PathTracer.render_camera; --spp only
// groups the samples between two pt_sync); only it allocates a ray buffer, and the two write byte-identical files.  pinhole is pt_render's camera (the same samples, bit for bit); thinlens takes --aperture R (lens radius in world units,
// default 0: everything sharp) and --focus D (distance of the plane in focus along front, default 35: the mirror sphere);
// ortho takes --ortho-height S (world height of the view volume, default 30: the sphere room's); fisheye takes --fisheye-deg A
// (full angle across the image circle, default 180; pixels outside the circle get --bk); equirect is the layout of --equirect,
// jittered.  Clamped mode when --out is a .png / .ppm, HDR when it is a .pfm, as --equirect; refused with --equirect and in the
// combinations --equirect is refused in (there are no guide buffers for these cameras).  --equirect itself keeps its host-made
// centre rays and its output.
// --adaptive E samples adaptively (the loop of gpu_pathtracer_amd.AdaptiveSampler): one pass of --pass-spp K samples (default 4) over
// every pixel through pt_render_pixels, then pt_select_pixels lists the pixels below --min-spp A, or whose relative standard error
// of the mean luminance is above E, and below --max-spp B, and pt_render_pixels gives those K more samples, until the list is
// empty.  A and B are multiples of K, K <= A <= B; --frames and --spp are not read.  Pass k renders frames k K .. k K + K - 1, so a
// pixel that ends with c samples holds exactly what a plain run of c samples gives it.  It works with --camera MODEL (not with
// --camera-loop); without --camera the model is the pinhole, pt_render's camera.  --out as for --camera: clamped for .png / .ppm,
// HDR for .pfm.  --samples-out writes the samples per pixel as a PFM (grey).  Refused in the combinations --camera is refused in.
// --env file.pfm lights the scene with a latitude-longitude radiance map (pt_upload_environment): a path that leaves the scene gathers
// the map along its direction instead of --bk.  The map lies in the world frame front = (0, 0, -1), right = (1, 0, 0), up = (0, 1, 0)
// — the frame of this app's camera, hence of the frames --equirect writes — and is looked up bilinearly (--env-nearest: the nearest
// texel); --env-scale S multiplies its texels.  With --gpus N every context gets it.  A checkpoint does not hold the map: pass --env
// again with --resume.  The probe round trip: render a probe of one scene,
//     pt_app --mesh room.ptmesh --equirect --width 512 --height 256 --out probe.pfm
// then light another mesh with it, usually without the reference's sphere room around it:
//     pt_app --mesh statue.ptmesh --no-spheres --env probe.pfm --out lit.png
// With a map the stage-split pipeline is not chosen (include/ptmi.h): the persistent kernel renders, the megakernel under --nee.
// --env-light also samples the map as a light (PT_OPT_ENV_LIGHT): every diffuse hit may send its shadow ray towards the map, drawn
// in proportion to the texels' brightness — what a map with a small, bright sun needs to converge.  It turns --nee on (next-event
// estimation with the cosine-weighted DIFF lobe, a miss keeping the path's light); a black map is lit by nothing and stays no light.
// --mis weighs next-event estimation's shadow rays against the bounce rays (PT_FLAG_MIS, the balance heuristic): it turns --nee on,
// and the megakernel renders.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptmi.h"
#include "pthost.h"

static int die(const char* what, const char* msg) {
    std::fprintf(stderr, "pt_app: %s: %s\n", what, msg ? msg : "");
    return 1;
}

int main(int argc, char** argv) {
    std::string mesh_path, out_path, ckpt_path, resume_path, denoise_path, variance_path, temporal_path, env_path;
    bool denoise_variance = false;
    double env_scale = 1.0;
    bool env_scale_set = false, env_nearest = false, env_light = false;
    int W = 1280, H = 720, frames = 16, depth = 4, mat = PT_MAT_DIFF, device = 0, spp = 1, ckpt_every = 0, gpus = 1, tile = 8;
    bool spheres = true, use_materials = true, device_build = false, fix_estimators = false, nee = false, mis = false, equirect = false;
    float bk[3] = {1.f, 1.f, 1.f};
    double until_error = -1.0;   // < 0: off
    long max_frames = -1;
    double pan_deg = 0.0, dolly = 0.0, spin_deg = 0.0;
    std::string camera_name;   // --camera: empty = pt_render's own pinhole
    bool camera_loop = false;  // --camera-loop: pt_camera_rays + pt_render_rays per sample instead of pt_render_camera
    double aperture = 0.0, focus = 35.0, ortho_height = 30.0, fisheye_deg = 180.0;
    double adaptive_error = -1.0;   // --adaptive: < 0 = off
    long min_spp = -1, max_spp = -1, pass_spp = 4;
    std::string samples_path;
    std::string tone_name, xfer_name, exposure_arg;   // --tonemap / --transfer / --exposure: any of them (or --white) sends the .png / .ppm outputs through pt_tonemap
    double white = INFINITY;
    bool white_set = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", name); std::exit(2); }
            return argv[++i];
        };
        if (a == "--mesh") mesh_path = next("--mesh");
        else if (a == "--out") out_path = next("--out");
        else if (a == "--denoise-out") denoise_path = next("--denoise-out");
        else if (a == "--denoise-variance") denoise_variance = true;
        else if (a == "--temporal-out") temporal_path = next("--temporal-out");
        else if (a == "--pan-deg") pan_deg = std::atof(next("--pan-deg"));
        else if (a == "--dolly") dolly = std::atof(next("--dolly"));
        else if (a == "--spin-deg") spin_deg = std::atof(next("--spin-deg"));
        else if (a == "--variance-out") variance_path = next("--variance-out");
        else if (a == "--until-error") until_error = std::atof(next("--until-error"));
        else if (a == "--max-frames") max_frames = std::atol(next("--max-frames"));
        else if (a == "--width") W = std::atoi(next("--width"));
        else if (a == "--height") H = std::atoi(next("--height"));
        else if (a == "--frames") frames = std::atoi(next("--frames"));
        else if (a == "--depth") depth = std::atoi(next("--depth"));
        else if (a == "--mat") mat = std::atoi(next("--mat"));
        else if (a == "--device") device = std::atoi(next("--device"));
        else if (a == "--no-spheres") spheres = false;
        else if (a == "--no-materials") use_materials = false;
        else if (a == "--device-build") device_build = true;
        else if (a == "--fix-estimators") fix_estimators = true;
        else if (a == "--nee") nee = true;   // next-event estimation (implies the cosine-weighted DIFF lobe and keeps a path's light on a miss)
        else if (a == "--mis") mis = true;   // ... with its shadow rays weighed against the bounce rays (implies --nee)
        else if (a == "--equirect") equirect = true;
        else if (a == "--camera") camera_name = next("--camera");
        else if (a == "--camera-loop") camera_loop = true;
        else if (a == "--aperture") aperture = std::atof(next("--aperture"));
        else if (a == "--focus") focus = std::atof(next("--focus"));
        else if (a == "--ortho-height") ortho_height = std::atof(next("--ortho-height"));
        else if (a == "--fisheye-deg") fisheye_deg = std::atof(next("--fisheye-deg"));
        else if (a == "--adaptive") adaptive_error = std::atof(next("--adaptive"));
        else if (a == "--min-spp") min_spp = std::atol(next("--min-spp"));
        else if (a == "--max-spp") max_spp = std::atol(next("--max-spp"));
        else if (a == "--pass-spp") pass_spp = std::atol(next("--pass-spp"));
        else if (a == "--samples-out") samples_path = next("--samples-out");
        else if (a == "--tonemap") tone_name = next("--tonemap");
        else if (a == "--transfer") xfer_name = next("--transfer");
        else if (a == "--exposure") exposure_arg = next("--exposure");
        else if (a == "--white") { white = std::atof(next("--white")); white_set = true; }
        else if (a == "--env") env_path = next("--env");
        else if (a == "--env-scale") { env_scale = std::atof(next("--env-scale")); env_scale_set = true; }
        else if (a == "--env-nearest") env_nearest = true;
        else if (a == "--env-light") env_light = true;
        else if (a == "--spp") spp = std::atoi(next("--spp"));
        else if (a == "--checkpoint") ckpt_path = next("--checkpoint");
        else if (a == "--checkpoint-every") ckpt_every = std::atoi(next("--checkpoint-every"));
        else if (a == "--resume") resume_path = next("--resume");
        else if (a == "--gpus") gpus = std::atoi(next("--gpus"));
        else if (a == "--tile") tile = std::atoi(next("--tile"));
        else if (a == "--bk") { for (int k = 0; k < 3; k++) bk[k] = (float)std::atof(next("--bk")); }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (mesh_path.empty()) return die("usage", "--mesh <file.obj|file.ptmesh> is required");
    if (spp < 1 || frames < 0 || W < 2 || H < 2) return die("usage", "--spp >= 1, --frames >= 0, --width/--height >= 2");
    if (gpus < 1 || gpus > 64 || tile < 8 || tile % 8) return die("usage", "--gpus 1..64, --tile a positive multiple of 8");
    // the display stage (pt_meter, pt_tonemap): off unless one of its flags is given
    const bool display = !tone_name.empty() || !xfer_name.empty() || !exposure_arg.empty() || white_set;
    const bool exposure_auto = exposure_arg == "auto";
    const int tone_curve = tone_name.empty() || tone_name == "clamp" ? PT_TONE_CLAMP : tone_name == "reinhard" ? PT_TONE_REINHARD : tone_name == "aces" ? PT_TONE_ACES : -1;
    const int tone_xfer = xfer_name.empty() || xfer_name == "linear" ? PT_XFER_LINEAR : xfer_name == "srgb" ? PT_XFER_SRGB : xfer_name == "gamma22" ? PT_XFER_GAMMA22 : -1;
    const double exposure = exposure_arg.empty() || exposure_auto ? 1.0 : std::atof(exposure_arg.c_str());
    if (tone_curve < 0) return die("--tonemap", "one of clamp, reinhard, aces");
    if (tone_xfer < 0) return die("--transfer", "one of linear, srgb, gamma22");
    if (!std::isfinite(exposure) || !(exposure > 0.0)) return die("--exposure", "a finite number > 0, or auto");
    if (white_set && !(white > 0.0)) return die("--white", "must be > 0");

    const bool until = until_error >= 0.0, with_moments = until || !variance_path.empty() || denoise_variance;
    if (denoise_variance && denoise_path.empty()) return die("usage", "--denoise-variance goes with --denoise-out");
    if (denoise_variance && (!temporal_path.empty() || !resume_path.empty()))
        return die("usage", "--denoise-variance does not combine with --temporal-out or --resume (neither keeps the moments of the samples)");
    if (until && max_frames < (long)frames) return die("usage", "--until-error needs --max-frames >= --frames");
    if (!until && max_frames >= 0) return die("usage", "--max-frames goes with --until-error");
    if (with_moments && !resume_path.empty()) return die("usage", "--variance-out / --until-error do not combine with --resume (a checkpoint holds no moments)");
    const bool spinning = spin_deg != 0.0;
    const bool moving = pan_deg != 0.0 || dolly != 0.0 || spinning, temporal = !temporal_path.empty();
    if (!std::isfinite(pan_deg) || !std::isfinite(dolly) || !std::isfinite(spin_deg)) return die("usage", "--pan-deg, --dolly and --spin-deg must be finite");
    if (temporal && (gpus > 1 || !resume_path.empty() || !ckpt_path.empty() || with_moments))
        return die("usage", "--temporal-out does not combine with --gpus > 1, --resume, --checkpoint, --variance-out or --until-error");
    if (moving && (!resume_path.empty() || !ckpt_path.empty() || until))
        return die("usage", "--pan-deg / --dolly / --spin-deg do not combine with --resume, --checkpoint or --until-error (a moving camera or mesh restarts the accumulation every frame)");
    if (equirect && (!denoise_path.empty() || temporal || with_moments || gpus > 1 || !ckpt_path.empty() || !resume_path.empty() || moving))
        return die("usage", "--equirect does not combine with --denoise-out, --temporal-out, --variance-out, --until-error, --gpus > 1, --checkpoint, --resume, --pan-deg, --dolly or --spin-deg (they need the pinhole frame)");
    // --camera: the model of pt_camera_rays; its own parameter is checked by the library at the first call
    const bool ray_camera = !camera_name.empty();
    pt_camera_model cmodel{};
    // --adaptive: pt_render_pixels / pt_select_pixels over the model's image, the pinhole without --camera
    const bool adaptive = adaptive_error >= 0.0;
    if (!adaptive && (min_spp >= 0 || max_spp >= 0 || pass_spp != 4 || !samples_path.empty()))
        return die("usage", "--min-spp, --max-spp, --pass-spp and --samples-out go with --adaptive E");
    if (adaptive) {
        if (!std::isfinite(adaptive_error)) return die("--adaptive", "the threshold must be finite and >= 0");
        if (pass_spp < 1 || min_spp < pass_spp || max_spp < min_spp || min_spp % pass_spp || max_spp % pass_spp || max_spp > 0x7fffffffL)
            return die("usage", "--adaptive needs --min-spp and --max-spp, multiples of --pass-spp with pass <= min <= max");
        if (camera_loop || equirect) return die("usage", "--adaptive does not combine with --camera-loop or --equirect");
        if (!denoise_path.empty() || temporal || with_moments || gpus > 1 || !ckpt_path.empty() || !resume_path.empty() || moving)
            return die("usage", "--adaptive does not combine with --denoise-out, --temporal-out, --variance-out, --until-error, --gpus > 1, --checkpoint, --resume, --pan-deg, --dolly or --spin-deg");
        cmodel.model = PT_CAM_PINHOLE; cmodel.width = W; cmodel.height = H;
    }
    if (camera_loop && !ray_camera) return die("usage", "--camera-loop needs --camera MODEL");
    if (ray_camera) {
        const char* names[5] = {"pinhole", "thinlens", "ortho", "fisheye", "equirect"};   // PT_CAM_* in order
        cmodel.model = -1;
        for (int k = 0; k < 5; k++)
            if (camera_name == names[k]) cmodel.model = k;
        if (cmodel.model < 0) return die("--camera", "one of pinhole, thinlens, ortho, fisheye, equirect");
        if (equirect) return die("usage", "--camera does not combine with --equirect (--camera equirect is its jittered form)");
        if (!denoise_path.empty() || temporal || with_moments || gpus > 1 || !ckpt_path.empty() || !resume_path.empty() || moving)
            return die("usage", "--camera does not combine with --denoise-out, --temporal-out, --variance-out, --until-error, --gpus > 1, --checkpoint, --resume, --pan-deg, --dolly or --spin-deg (they need pt_render's pinhole frame)");
        cmodel.width = W; cmodel.height = H;
        cmodel.lens_radius = (float)aperture; cmodel.focus_dist = (float)focus;
        cmodel.ortho_height = (float)ortho_height;
        cmodel.fisheye_fov = (float)(fisheye_deg * 3.14159265358979323846 / 180.0);
    }

    // --env: the map is read and checked before anything is built or rendered
    int env_w = 0, env_h = 0;
    float* env_px = nullptr;
    if (env_path.empty() && env_scale_set) return die("--env-scale", "goes with --env");
    if (env_path.empty() && env_nearest) return die("--env-nearest", "goes with --env");
    if (env_path.empty() && env_light) return die("--env-light", "goes with --env");
    if (env_light) nee = true;   // the map is one of next-event estimation's lights
    if (mis) nee = true;
    if (!env_path.empty()) {
        if (!std::isfinite(env_scale) || env_scale < 0.0) return die("--env-scale", "must be finite and not negative");
        if (pth_read_pfm(env_path.c_str(), &env_w, &env_h, &env_px) != 0) return die("--env", pth_last_error());
        if (env_w > 16384 || env_h > 16384 || (uint64_t)env_w * (uint64_t)env_h > (1ull << 26)) return die("--env", "the map is larger than 16384 texels a side or 2^26 texels");
    }

    const bool is_ptmesh = mesh_path.size() > 7 && mesh_path.substr(mesh_path.size() - 7) == ".ptmesh";
    pth_mesh* mesh = is_ptmesh ? pth_mesh_load_ptmesh(mesh_path.c_str()) : pth_mesh_load_obj(mesh_path.c_str());
    if (!mesh) return die("mesh", pth_last_error());
    // one context per GPU of the tile split (ctxs[0] = `ctx` is where the merged frame is assembled from)
    const int n_dev = pt_device_count();
    if (n_dev < 1) return die("pt_device_count", pt_last_error(nullptr));
    std::vector<pt_ctx*> ctxs((size_t)gpus, nullptr);
    for (int g = 0; g < gpus; g++)
        if (pt_create((device + g) % n_dev, &ctxs[(size_t)g]) != PT_OK) return die("pt_create", pt_last_error(nullptr));
    pt_ctx* ctx = ctxs[0];
    if (gpus > 1) std::printf("tile split over %d context(s) on %d device(s), stripes of %d rows\n", gpus, std::min(gpus, n_dev), tile);
    pth_bvh* bvh = nullptr;
    if (!device_build) {
        bvh = pth_bvh_build(mesh, nullptr);
        if (!bvh) return die("bvh", pth_last_error());
        pth_bvh_stats st;
        pth_bvh_get_stats(bvh, &st);
        std::printf("mesh %zu tris; bvh %llu inner, %llu leaves, depth %u, built in %.1f ms\n", pth_mesh_n_tris(mesh),
                    (unsigned long long)st.n_inner, (unsigned long long)st.n_leaves, st.max_depth, st.build_ms);
    }
    const bool has_materials = use_materials && pth_mesh_n_materials(mesh) > 0;
    for (pt_ctx* cx : ctxs) {   // the scene is replicated: every GPU needs all of it for its own pixels
        if (device_build) {
            if (pt_build_bvh(cx, pth_mesh_verts(mesh), pth_mesh_n_verts(mesh), pth_mesh_tris(mesh), pth_mesh_n_tris(mesh)) != PT_OK)
                return die("pt_build_bvh", pt_last_error(cx));
            float bms = 0.f;
            pt_last_build_ms(cx, &bms);
            if (cx == ctx) std::printf("mesh %zu tris; bvh built on the device in %.2f ms\n", pth_mesh_n_tris(mesh), bms);
        } else if (pt_upload_bvh(cx, pth_bvh_nodes(bvh), pth_bvh_n_node_vec4(bvh), pth_bvh_tris(bvh), pth_bvh_n_tri_vec4(bvh),
                                 pth_bvh_index(bvh), pth_bvh_n_index(bvh)) != PT_OK) {
            return die("pt_upload_bvh", pt_last_error(cx));
        }
        if (has_materials) {
            static_assert(sizeof(pth_material) == sizeof(pt_material), "one layout");
            if (pt_upload_tri_materials(cx, (const pt_material*)pth_mesh_materials(mesh), pth_mesh_n_materials(mesh),
                                        pth_mesh_tri_materials(mesh), pth_mesh_n_tris(mesh)) != PT_OK)
                return die("pt_upload_tri_materials", pt_last_error(cx));
        }
    }
    if (has_materials) std::printf("%zu materials from the mesh file\n", pth_mesh_n_materials(mesh));
    if (env_px) {   // the map in the world frame, on every context
        pt_environment ev{};
        ev.width = env_w; ev.height = env_h;
        ev.front[2] = -1.f; ev.right[0] = 1.f; ev.up[1] = 1.f;
        ev.scale[0] = ev.scale[1] = ev.scale[2] = (float)env_scale;
        ev.filter = env_nearest ? PT_ENV_NEAREST : PT_ENV_BILINEAR;
        int is_light = 0;
        for (pt_ctx* cx : ctxs) {
            if (pt_set_option(cx, PT_OPT_ENV_LIGHT, env_light ? 1 : 0) != PT_OK) return die("--env-light", pt_last_error(cx));
            if (pt_upload_environment(cx, &ev, env_px) != PT_OK) return die("--env", pt_last_error(cx));
            if (pt_environment_is_light(cx, &is_light) != PT_OK) return die("--env-light", pt_last_error(cx));
        }
        pth_free_pfm(env_px);
        env_px = nullptr;
        std::printf("environment map %s: %d x %d, %s%s\n", env_path.c_str(), env_w, env_h, env_nearest ? "nearest" : "bilinear",
                    is_light ? ", sampled as a light" : env_light ? ", black: not a light" : "");
    }

    // the reference's sphere room, BasicScene.cpp:181-202
    std::vector<pt_sphere> sph;
    if (spheres) {
        const float rad = 600.f, px = 20.f, py = 15.f;
        const float a[3] = {197.f / 255.f, 153.f / 255.f, 92.f / 255.f};
        auto add = [&](float x, float y, float z, float r, const float* e, float cr, float cg, float cb, int m) {
            pt_sphere s{{x, y, z, r}, {e[0], e[1], e[2]}, {cr, cg, cb}, m};
            sph.push_back(s);
        };
        const float red[3] = {165.f / 255.f, 15.f / 255.f, 0.f}, green[3] = {30.f / 255.f, 76.f / 255.f, 14.f / 255.f};
        const float cyan[3] = {0.f, 1.f, 0.8f}, zero[3] = {0, 0, 0}, lamp[3] = {0.f, 1.f, 1.f};
        add(0, -py - rad, -20, rad, a, .5f, .5f, .5f, PT_MAT_DIFF);
        add(0, py + rad, -20, rad, a, .1f, .3f, .4f, PT_MAT_DIFF);
        add(px + rad, 0, -20, rad, red, red[0], red[1], red[2], PT_MAT_DIFF);
        add(-px - rad, 0, -20, rad, green, green[0], green[1], green[2], PT_MAT_DIFF);
        add(0, 0, -rad * 1.5f - 20, rad, a, 1, 1, 1, PT_MAT_DIFF);
        add(0, 0, rad * 1.5f + 20, rad, cyan, .5f, .5f, .5f, PT_MAT_DIFF);
        add(13, -8, -35, 6, zero, 1, 1, 1, PT_MAT_SPEC);
        add(10, -15, -68, 10, lamp, 1, 1, 1, PT_MAT_DIFF);
        for (pt_ctx* cx : ctxs)
            if (pt_upload_spheres(cx, sph.data(), sph.size()) != PT_OK) return die("pt_upload_spheres", pt_last_error(cx));
    }

    // kernel defaults (BasicScene.cpp:220-236) and camera (:239-259)
    pt_camera cam{};
    cam.front[2] = -1.f; cam.right[0] = 1.f; cam.up[1] = 1.f;
    cam.dist = (float)(H / 60);
    cam.aspect = W * 1.0f / H;
    cam.fov = 1.0f;
    pt_params p{};
    p.width = W; p.height = H; p.depth = (uint32_t)depth; p.cull_backfaces = 1;
    p.tri_mat = mat;
    p.tri_col[0] = 246.f / 256.f; p.tri_col[1] = 246.f / 255.f; p.tri_col[2] = 70.f / 255.f;
    p.bk_color[0] = bk[0]; p.bk_color[1] = bk[1]; p.bk_color[2] = bk[2];
    p.air_ior = 1.0f; p.glass_ior = 1.4f; p.phong_expo = 30.f;
    p.flags = PT_FLAG_WRITE_RGBA;
    if (fix_estimators) p.flags |= PT_FLAG_FACE_FORWARD | PT_FLAG_COSINE_DIFF | PT_FLAG_GLASS_FIX | PT_FLAG_RUSSIAN_ROULETTE;
    if (nee) p.flags |= PT_FLAG_COSINE_DIFF | PT_FLAG_NEE | PT_FLAG_MISS_KEEPS_PATH;
    if (mis) p.flags |= PT_FLAG_MIS;
    p.part_count = gpus; p.part_rows = tile;

    // every context owns full-frame buffers (accum/rgba are always addressed by the global pixel); it touches only
    // its own stripes of them
    std::vector<void*> accums((size_t)gpus, nullptr), rgbas((size_t)gpus, nullptr);
    for (int g = 0; g < gpus; g++) {
        if (pt_malloc(ctxs[(size_t)g], (size_t)W * H * 12, &accums[(size_t)g]) != PT_OK || pt_malloc(ctxs[(size_t)g], (size_t)W * H * 4, &rgbas[(size_t)g]) != PT_OK)
            return die("pt_malloc", pt_last_error(ctxs[(size_t)g]));
        pt_memset(ctxs[(size_t)g], accums[(size_t)g], 0, (size_t)W * H * 12);
    }
    void *accum = accums[0], *rgba = rgbas[0];
    // the luminance moments of every context's stripes (pt_render_moments), and on the first context a buffer for the gathered ones
    std::vector<void*> moments((size_t)gpus, nullptr);
    void* moments_all = nullptr;
    if (with_moments) {
        for (int g = 0; g < gpus; g++)
            if (pt_malloc(ctxs[(size_t)g], (size_t)W * H * 8, &moments[(size_t)g]) != PT_OK) return die("pt_malloc", pt_last_error(ctxs[(size_t)g]));
        moments_all = moments[0];
        if (gpus > 1 && until && pt_malloc(ctx, (size_t)W * H * 8, &moments_all) != PT_OK) return die("pt_malloc", pt_last_error(ctx));
    }
    // gather: rows of stripe s belong to context s % gpus; `elem` bytes per pixel
    std::vector<unsigned char> part_buf;
    auto gather = [&](std::vector<void*>& dev, void* host, size_t elem) -> int {
        if (pt_download(ctxs[0], host, dev[0], (size_t)W * H * elem) != PT_OK) return die("pt_download", pt_last_error(ctxs[0]));
        for (int g = 1; g < gpus; g++) {
            part_buf.resize((size_t)W * H * elem);
            if (pt_download(ctxs[(size_t)g], part_buf.data(), dev[(size_t)g], part_buf.size()) != PT_OK) return die("pt_download", pt_last_error(ctxs[(size_t)g]));
            for (int s0 = g * tile; s0 < H; s0 += gpus * tile) {
                const size_t off = (size_t)s0 * W * elem, len = (size_t)std::min(tile, H - s0) * W * elem;
                std::memcpy((unsigned char*)host + off, part_buf.data() + off, len);
            }
        }
        return 0;
    };

    // what a checkpoint must agree on to be continued: geometry size, image size, the scalar parameters
    uint64_t tag = pth_frame_hash((uint64_t)pth_mesh_n_tris(mesh) * 1315423911ull + (uint64_t)W * 65537u + (uint64_t)H);
    tag = pth_frame_hash(tag ^ ((uint64_t)depth << 32 | (uint64_t)mat << 8 | (fix_estimators ? 4u : 0u) | (nee ? 8u : 0u) | (mis ? 16u : 0u) | (spheres ? 2u : 0u) | (has_materials ? 1u : 0u)));

    uint64_t frameNumber = 0, constantPdf = 0;   // constantPdf = samples folded so far
    std::vector<float> host_acc;
    if (!resume_path.empty()) {
        pth_checkpoint_info ci{};
        host_acc.resize((size_t)W * H * 3);
        if (pth_checkpoint_load(resume_path.c_str(), &ci, nullptr) != 0) return die("resume", pth_last_error());
        if (ci.width != W || ci.height != H || ci.scene_tag != tag) return die("resume", "checkpoint belongs to another scene / image size / parameters");
        if (pth_checkpoint_load(resume_path.c_str(), &ci, host_acc.data()) != 0) return die("resume", pth_last_error());
        for (int g = 0; g < gpus; g++)   // every context continues its own stripes
            if (pt_upload(ctxs[(size_t)g], accums[(size_t)g], host_acc.data(), host_acc.size() * 4) != PT_OK) return die("pt_upload", pt_last_error(ctxs[(size_t)g]));
        frameNumber = ci.next_frame;
        constantPdf = ci.constant_pdf;
        std::printf("resumed %s: %llu samples per pixel done\n", resume_path.c_str(), (unsigned long long)constantPdf);
    }
    auto save_checkpoint = [&]() -> int {
        host_acc.resize((size_t)W * H * 3);
        if (int rc = gather(accums, host_acc.data(), 12)) return rc;
        pth_checkpoint_info ci{W, H, frameNumber, constantPdf, tag};
        if (pth_checkpoint_save(ckpt_path.c_str(), &ci, host_acc.data()) != 0) return die("checkpoint", pth_last_error());
        return 0;
    };

    // --temporal-out: the ping-pong history (colour, length, guides) of TemporalHistory, on the one context
    const size_t n_pix_all = (size_t)W * H;
    void *t_color[2] = {nullptr, nullptr}, *t_len[2] = {nullptr, nullptr}, *t_alb[2] = {nullptr, nullptr}, *t_nrm[2] = {nullptr, nullptr},
         *t_pos[2] = {nullptr, nullptr}, *t_id[2] = {nullptr, nullptr}, *t_rgba = nullptr;
    int t_cur = 0;          // the set the next push writes
    bool t_has = false;     // a history exists
    pt_camera t_cam{};      // its camera
    const pt_temporal_params tpar = {W, H, 32.0f, 0.02f, 0.9f, 0};   // = gpu_pathtracer_amd.TEMPORAL_DEFAULTS
    if (temporal) {
        for (int k = 0; k < 2; k++)
            if (pt_malloc(ctx, n_pix_all * 12, &t_color[k]) != PT_OK || pt_malloc(ctx, n_pix_all * 4, &t_len[k]) != PT_OK ||
                pt_malloc(ctx, n_pix_all * 16, &t_alb[k]) != PT_OK || pt_malloc(ctx, n_pix_all * 16, &t_nrm[k]) != PT_OK ||
                pt_malloc(ctx, n_pix_all * 16, &t_pos[k]) != PT_OK || (spinning && pt_malloc(ctx, n_pix_all * 4, &t_id[k]) != PT_OK))
                return die("pt_malloc", pt_last_error(ctx));
        if (pt_malloc(ctx, n_pix_all * 4, &t_rgba) != PT_OK) return die("pt_malloc", pt_last_error(ctx));
    }
    // --spin-deg: the rest pose as rows v0, v1, v2 by triangle id, and per context two device vertex buffers (pt_refit_bvh's layout);
    // displayed frame f is rendered from buffer f & 1, so the buffer of the frame before it is still whole when the history reads it
    const size_t n_spin_tris = pth_mesh_n_tris(mesh);
    std::vector<double> spin_rest;
    std::vector<float> spin_rows;
    double spin_c[3] = {0.0, 0.0, 0.0};
    std::vector<void*> spin_buf((size_t)gpus * 2, nullptr);
    if (spinning) {
        const float* mv = pth_mesh_verts(mesh);
        const int32_t* mt = pth_mesh_tris(mesh);
        spin_rest.resize(n_spin_tris * 9);
        spin_rows.resize(n_spin_tris * 9);
        for (size_t i = 0; i < n_spin_tris * 3; i++)
            for (int a = 0; a < 3; a++) spin_rest[3 * i + a] = (double)mv[3 * (size_t)mt[i] + a];
        float lo[3], hi[3];
        pth_mesh_bounds(mesh, lo, hi);
        for (int a = 0; a < 3; a++) spin_c[a] = 0.5 * ((double)lo[a] + (double)hi[a]);
        for (size_t i = 0; i < spin_rest.size(); i++) spin_rows[i] = (float)spin_rest[i];
        for (int g = 0; g < gpus; g++)
            for (int b = 0; b < 2; b++)
                if (pt_malloc(ctxs[(size_t)g], spin_rows.size() * 4, &spin_buf[(size_t)g * 2 + b]) != PT_OK ||
                    pt_upload(ctxs[(size_t)g], spin_buf[(size_t)g * 2 + b], spin_rows.data(), spin_rows.size() * 4) != PT_OK)
                    return die("--spin-deg", pt_last_error(ctxs[(size_t)g]));
    }
    auto spin_mesh = [&](int f) -> int {   // the mesh of displayed frame f: the rest pose turned by f x spin_deg about (0, 1, 0) through spin_c
        const double th = spin_deg * (double)f * 3.14159265358979323846 / 180.0, cs = std::cos(th), sn = std::sin(th);
        for (size_t i = 0; i < n_spin_tris * 3; i++) {
            const double x = spin_rest[3 * i] - spin_c[0], z = spin_rest[3 * i + 2] - spin_c[2];
            spin_rows[3 * i] = (float)(spin_c[0] + cs * x + sn * z);
            spin_rows[3 * i + 1] = (float)spin_rest[3 * i + 1];
            spin_rows[3 * i + 2] = (float)(spin_c[2] - sn * x + cs * z);
        }
        for (int g = 0; g < gpus; g++) {
            void* buf = spin_buf[(size_t)g * 2 + (f & 1)];
            if (pt_upload(ctxs[(size_t)g], buf, spin_rows.data(), spin_rows.size() * 4) != PT_OK) return die("--spin-deg", pt_last_error(ctxs[(size_t)g]));
            if (pt_refit_bvh(ctxs[(size_t)g], (const float*)buf, n_spin_tris, nullptr) != PT_OK) return die("pt_refit_bvh", pt_last_error(ctxs[(size_t)g]));
        }
        return 0;
    };
    int calls = 0;
    auto temporal_push = [&]() -> int {   // guides of `cam`, the frame in `accum` against the history, swap
        const int k = t_cur, o = 1 - t_cur;
        if (pt_render_aux(ctx, &cam, &p, (float*)t_alb[k], (float*)t_nrm[k], (float*)t_pos[k], (int32_t*)t_id[k]) != PT_OK) return die("pt_render_aux", pt_last_error(ctx));
        if (spinning) {   // the frame just rendered is number calls - 1: its vertices and those of the frame before it
            const int f = calls - 1;
            if (pt_temporal_motion(ctx, &tpar, t_has ? &t_cam : nullptr, (const float*)spin_buf[(size_t)(1 - (f & 1))], (const float*)spin_buf[(size_t)(f & 1)],
                                   n_spin_tris, t_has ? (const float*)t_color[o] : nullptr, (const float*)t_len[o], (const float*)t_nrm[o],
                                   (const float*)t_pos[o], (const int32_t*)t_id[o], (const float*)accum, (const float*)t_nrm[k], (const float*)t_pos[k],
                                   (const int32_t*)t_id[k], (float*)t_color[k], (float*)t_len[k], (uint32_t*)t_rgba, nullptr) != PT_OK)
                return die("pt_temporal_motion", pt_last_error(ctx));
        } else if (pt_temporal(ctx, &tpar, t_has ? &t_cam : nullptr, t_has ? (const float*)t_color[o] : nullptr, (const float*)t_len[o],
                        (const float*)t_nrm[o], (const float*)t_pos[o], nullptr, (const float*)accum, (const float*)t_nrm[k],
                        (const float*)t_pos[k], nullptr, (float*)t_color[k], (float*)t_len[k], (uint32_t*)t_rgba) != PT_OK)
            return die("pt_temporal", pt_last_error(ctx));
        t_cam = cam;
        t_has = true;
        t_cur = o;
        return 0;
    };
    // the camera of displayed frame k: the first one turned by k x pan_deg about up (from the first basis, in double: no drift),
    // pos moved `dolly` along each frame's front in turn
    const pt_camera cam0 = cam;
    double cam_pos[3] = {cam.pos[0], cam.pos[1], cam.pos[2]};
    auto move_camera = [&](int k) {
        const double th = pan_deg * (double)k * 3.14159265358979323846 / 180.0, cs = std::cos(th), sn = std::sin(th);
        const double u[3] = {cam0.up[0], cam0.up[1], cam0.up[2]};
        auto rot = [&](const float* v, float* out) {   // Rodrigues: v cos + (u x v) sin + u (u . v)(1 - cos)
            const double x[3] = {v[0], v[1], v[2]};
            const double cr[3] = {u[1] * x[2] - u[2] * x[1], u[2] * x[0] - u[0] * x[2], u[0] * x[1] - u[1] * x[0]};
            const double ud = u[0] * x[0] + u[1] * x[1] + u[2] * x[2];
            for (int i = 0; i < 3; i++) out[i] = (float)(x[i] * cs + cr[i] * sn + u[i] * ud * (1.0 - cs));
        };
        rot(cam0.front, cam.front);
        rot(cam0.right, cam.right);
        for (int i = 0; i < 3; i++) { cam_pos[i] += dolly * (double)cam.front[i]; cam.pos[i] = (float)cam_pos[i]; }
    };

    // --equirect: the latitude-longitude rays of the pixels, float[H W][8], made once (the camera stands still)
    void* eq_rays = nullptr;
    const bool out_pfm = out_path.size() > 4 && out_path.substr(out_path.size() - 4) == ".pfm";
    const bool out_hdr = out_pfm || display;   // the ray routes keep the unclamped mean for a .pfm and for the display stage, whose curve does the clamping
    if (equirect) {
        const double pi = 3.14159265358979323846;
        std::vector<float> rays((size_t)W * H * 8, 0.f);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const double lon = (x - W / 2.0) * 2.0 * pi / W, lat = (y - H / 2.0) * pi / H;
                double d[3], len = 0.0;
                for (int i = 0; i < 3; i++) {
                    d[i] = std::cos(lat) * (std::cos(lon) * cam.front[i] + std::sin(lon) * cam.right[i]) + std::sin(lat) * cam.up[i];
                    len += d[i] * d[i];
                }
                float* r = &rays[((size_t)y * W + x) * 8];
                for (int i = 0; i < 3; i++) { r[i] = cam.pos[i]; r[4 + i] = (float)(d[i] / std::sqrt(len)); }
            }
        if (pt_malloc(ctx, rays.size() * 4, &eq_rays) != PT_OK || pt_upload(ctx, eq_rays, rays.data(), rays.size() * 4) != PT_OK)
            return die("equirect rays", pt_last_error(ctx));
    }
    // --camera --camera-loop: the buffer pt_camera_rays fills for every sample, float[H W][8]
    if (ray_camera && camera_loop && pt_malloc(ctx, (size_t)W * H * 32, &eq_rays) != PT_OK) return die("camera rays", pt_last_error(ctx));

    const uint64_t first_frame = frameNumber;
    uint64_t end_frame = frameNumber + (uint64_t)frames;
    const uint64_t last_frame = until ? frameNumber + (uint64_t)max_frames : end_frame;   // --until-error: never past --max-frames
    std::vector<float> host_mom;
    double mean_rse = -1.0;   // pt_frame_error's figure after the last call, < 0: not computed (fewer than two samples)
    auto t0 = std::chrono::steady_clock::now();
    if (adaptive) {   // gpu_pathtracer_amd.AdaptiveSampler.run
        void *a_mom = nullptr, *a_cnt = nullptr, *a_pix = nullptr;
        if (pt_malloc(ctx, n_pix_all * 8, &a_mom) != PT_OK || pt_malloc(ctx, n_pix_all * 4, &a_cnt) != PT_OK || pt_malloc(ctx, n_pix_all * 4, &a_pix) != PT_OK ||
            pt_memset(ctx, a_cnt, 0, n_pix_all * 4) != PT_OK)
            return die("pt_malloc", pt_last_error(ctx));
        const pt_select_params sel = {W, H, (float)adaptive_error, (uint32_t)min_spp, (uint32_t)max_spp, 0};
        const int mode = out_hdr ? PT_RAYS_HDR : PT_RAYS_CLAMPED;
        uint64_t n_sel = n_pix_all, total = 0;
        p.sample_index = 1;   // (not read: the counts carry N)
        for (const uint32_t* list = nullptr;; list = (const uint32_t*)a_pix) {
            p.frame = first_frame + (uint64_t)calls * (uint64_t)pass_spp;
            if (pt_render_pixels(ctx, &cam, &cmodel, list, (size_t)n_sel, (float*)accum, (float*)a_mom, (uint32_t*)a_cnt, &p, (uint32_t)pass_spp, mode) != PT_OK)
                return die("pt_render_pixels", pt_last_error(ctx));
            total += n_sel * (uint64_t)pass_spp;
            calls++;
            if (pt_select_pixels(ctx, &sel, (const float*)a_mom, (const uint32_t*)a_cnt, (uint32_t*)a_pix, &n_sel, &mean_rse) != PT_OK)
                return die("pt_select_pixels", pt_last_error(ctx));
            if (n_sel == 0) break;
        }
        std::printf("adaptive %g: %d passes, %llu samples, %.3f per pixel (min %ld, max %ld), mean_rse %.6g\n", adaptive_error, calls,
                    (unsigned long long)total, (double)total / (double)n_pix_all, min_spp, max_spp, mean_rse);
        frameNumber = first_frame + (uint64_t)((total + n_pix_all - 1) / n_pix_all);   // for the summary line: the mean, rounded up
        if (!samples_path.empty()) {
            std::vector<uint32_t> cnt(n_pix_all);
            if (pt_download(ctx, cnt.data(), a_cnt, n_pix_all * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
            std::vector<float> img(n_pix_all * 3);
            for (size_t i = 0; i < n_pix_all; i++) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = (float)cnt[i];
            if (pth_write_pfm(samples_path.c_str(), img.data(), W, H) != 0) return die("write", pth_last_error());
        }
        for (void* b : {a_mom, a_cnt, a_pix}) pt_free(ctx, b);
    }
    for (; !adaptive;) {
        while (frameNumber < end_frame) {
            for (pt_ctx* cx : ctxs)
                if (pt_sync(cx) != PT_OK) return die("pt_sync", pt_last_error(cx));     // :395
            const uint32_t n = (uint32_t)std::min<uint64_t>((uint64_t)spp, end_frame - frameNumber);
            if (moving && calls > 0) move_camera(calls);                                // the camera is dirty: start over (:399)
            if (spinning && calls > 0)
                if (int rc = spin_mesh(calls)) return rc;
            p.frame = frameNumber;                                                      // :397
            p.sample_index = moving ? 1 : constantPdf + 1;                              // :399 (1 on the first frame: overwrite)
            if (equirect) {
                if (pt_render_rays(ctx, (const float*)eq_rays, (size_t)W * H, 0, (float*)accum, &p, n, out_hdr ? PT_RAYS_HDR : PT_RAYS_CLAMPED) != PT_OK)
                    return die("pt_render_rays", pt_last_error(ctx));
            } else if (ray_camera && !camera_loop) {   // a fresh jittered ray per sample, made where its path starts
                if (pt_render_camera(ctx, &cam, &cmodel, nullptr, (size_t)W * H, 0, (float*)accum, &p, n, out_hdr ? PT_RAYS_HDR : PT_RAYS_CLAMPED) != PT_OK)
                    return die("pt_render_camera", pt_last_error(ctx));
            } else if (ray_camera) {   // the same samples by their definition: generate, trace, on one stream
                pt_params q = p;
                for (uint32_t s = 0; s < n; s++) {
                    q.frame = p.frame + s; q.sample_index = p.sample_index + s;
                    if (pt_camera_rays(ctx, &cam, &cmodel, q.frame, nullptr, (size_t)W * H, 0, (float*)eq_rays) != PT_OK)
                        return die("pt_camera_rays", pt_last_error(ctx));
                    if (pt_render_rays(ctx, (const float*)eq_rays, (size_t)W * H, 0, (float*)accum, &q, 1, out_hdr ? PT_RAYS_HDR : PT_RAYS_CLAMPED) != PT_OK)
                        return die("pt_render_rays", pt_last_error(ctx));
                }
            } else
            for (int g = 0; g < gpus; g++) {                                            // :404, once per GPU: asynchronous, so the GPUs run side by side
                p.part_index = g;
                if (pt_render_moments(ctxs[(size_t)g], (float*)accums[(size_t)g], (uint32_t*)rgbas[(size_t)g], (float*)moments[(size_t)g], &cam, &p, n) != PT_OK)
                    return die("pt_render", pt_last_error(ctxs[(size_t)g]));
            }
            frameNumber += n;
            constantPdf = moving ? n : constantPdf + n;
            calls++;
            if (temporal && moving)
                if (int rc = temporal_push()) return rc;
            if (!ckpt_path.empty() && ckpt_every > 0 && calls % ckpt_every == 0 && frameNumber < end_frame)
                if (int rc = save_checkpoint()) return rc;
        }
        if (!until) break;
        if (constantPdf >= 2) {   // the frame's error so far: the stripes' moments gathered onto the first context
            if (gpus > 1) {
                host_mom.resize((size_t)W * H * 2);
                if (int grc = gather(moments, host_mom.data(), 8)) return grc;
                if (pt_upload(ctx, moments_all, host_mom.data(), host_mom.size() * 4) != PT_OK) return die("pt_upload", pt_last_error(ctx));
            }
            if (pt_frame_error(ctx, (const float*)moments_all, W, H, constantPdf, 0.f, &mean_rse, nullptr) != PT_OK)
                return die("pt_frame_error", pt_last_error(ctx));
            if (mean_rse <= until_error) break;
        }
        if (frameNumber >= last_frame) break;
        end_frame = std::min<uint64_t>(frameNumber + (uint64_t)spp, last_frame);
    }
    frames = (int)(frameNumber - first_frame);   // what was rendered: more than asked for under --until-error
    if (temporal && !t_has)   // the camera stood still: the accumulator is the one frame of the history
        if (int rc = temporal_push()) return rc;
    if (until) std::printf("until-error %g: %d frames rendered, mean_rse %.6g\n", until_error, frames, mean_rse);
    for (pt_ctx* cx : ctxs) pt_sync(cx);
    double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const double rays = (double)W * H * depth * frames;
    std::printf("%d samples/pixel %dx%d depth %d in %d calls: %.2f ms/sample, <= %.1f Mrays/s (closed scene bound)\n", frames, W, H,
                depth, calls, frames ? ms / frames : 0.0, ms > 0 ? rays / ms / 1e3 : 0.0);
    if (!ckpt_path.empty())
        if (int rc = save_checkpoint()) return rc;

    // --tonemap / --transfer / --exposure / --white: a float[H][W][3] buffer of the first context into display words, on the device —
    // pt_meter first under --exposure auto (key 0.18 over every metered pixel; the exposure never leaves the device), then pt_tonemap
    void *tone_rgba = nullptr, *tone_state = nullptr;
    auto display_words = [&](const void* color_dev, std::vector<uint32_t>& img) -> int {
        if (!tone_rgba && pt_malloc(ctx, img.size() * 4, &tone_rgba) != PT_OK) return die("pt_malloc", pt_last_error(ctx));
        if (exposure_auto) {
            if (!tone_state && (pt_malloc(ctx, 16, &tone_state) != PT_OK || pt_memset(ctx, tone_state, 0, 16) != PT_OK)) return die("pt_malloc", pt_last_error(ctx));
            const pt_meter_params mp = {W, H, 0.18f, 0.0f, 1.0f, 1.0f / 65536.0f, 65536.0f, 1.0f};
            if (pt_meter(ctx, &mp, (const float*)color_dev, (float*)tone_state, 1) != PT_OK) return die("pt_meter", pt_last_error(ctx));
        }
        const pt_tonemap_params tp = {W, H, tone_curve, tone_xfer, (float)exposure, (float)white};
        if (pt_tonemap(ctx, &tp, (const float*)color_dev, exposure_auto ? (const float*)tone_state : nullptr, nullptr, (uint32_t*)tone_rgba) != PT_OK)
            return die("pt_tonemap", pt_last_error(ctx));
        if (pt_download(ctx, img.data(), tone_rgba, img.size() * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
        return 0;
    };
    if (!out_path.empty()) {
        const std::string ext = out_path.size() > 4 ? out_path.substr(out_path.size() - 4) : std::string();
        int rc;
        if (ext == ".pfm") {
            host_acc.resize((size_t)W * H * 3);
            if (int grc = gather(accums, host_acc.data(), 12)) return grc;
            rc = pth_write_pfm(out_path.c_str(), host_acc.data(), W, H);
        } else {
            std::vector<uint32_t> img((size_t)W * H);
            if (display) {   // the accumulator through pt_tonemap on the first context (the other contexts' stripes gathered into a buffer of it)
                void* color = accum;
                if (gpus > 1) {
                    host_acc.resize((size_t)W * H * 3);
                    if (int grc = gather(accums, host_acc.data(), 12)) return grc;
                    if (pt_malloc(ctx, host_acc.size() * 4, &color) != PT_OK || pt_upload(ctx, color, host_acc.data(), host_acc.size() * 4) != PT_OK)
                        return die("pt_upload", pt_last_error(ctx));
                }
                if (int drc = display_words(color, img)) return drc;
                if (gpus > 1) pt_free(ctx, color);
            } else if (frames == 0 || equirect || ray_camera || adaptive) {  // nothing rendered in this run (e.g. --resume only to convert), or no display words (pt_render_rays): pack the accumulator here
                host_acc.resize((size_t)W * H * 3);
                if (int grc = gather(accums, host_acc.data(), 12)) return grc;
                for (size_t i = 0; i < img.size(); i++) {   // rgbToUint, cudaUtils.h:99-105
                    auto q = [&](float v) { v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v); return (uint32_t)(v * 255.f); };
                    img[i] = q(host_acc[3 * i]) | (q(host_acc[3 * i + 1]) << 8) | (q(host_acc[3 * i + 2]) << 16);
                }
            } else if (int grc = gather(rgbas, img.data(), 4)) {
                return grc;
            }
            rc = ext == ".png" ? pth_write_png(out_path.c_str(), img.data(), W, H) : pth_write_ppm(out_path.c_str(), img.data(), W, H);
        }
        if (rc != 0) return die("write", pth_last_error());
    }
    if (!variance_path.empty()) {   // variance of the mean luminance per pixel from the gathered moments
        if (constantPdf < 2) return die("variance-out", "needs at least two samples per pixel");
        const size_t n_pix = (size_t)W * H;
        host_mom.resize(n_pix * 2);
        if (int grc = gather(moments, host_mom.data(), 8)) return grc;
        std::vector<float> img(n_pix * 3);
        const float nm1 = (float)(constantPdf - 1);
        for (size_t i = 0; i < n_pix; i++) {
            const float m1 = host_mom[2 * i], m2 = host_mom[2 * i + 1];
            img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = std::max(0.f, m2 - m1 * m1) / nm1;
        }
        if (pth_write_pfm(variance_path.c_str(), img.data(), W, H) != 0) return die("write", pth_last_error());
    }
    if (temporal) {   // the history after the last frame
        const int k = 1 - t_cur;
        const std::string ext = temporal_path.size() > 4 ? temporal_path.substr(temporal_path.size() - 4) : std::string();
        int rc;
        if (ext == ".pfm") {
            std::vector<float> img(n_pix_all * 3);
            if (pt_download(ctx, img.data(), t_color[k], img.size() * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
            rc = pth_write_pfm(temporal_path.c_str(), img.data(), W, H);
        } else {
            std::vector<uint32_t> img(n_pix_all);
            if (display) {
                if (int drc = display_words(t_color[k], img)) return drc;
            } else if (pt_download(ctx, img.data(), t_rgba, img.size() * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
            rc = ext == ".png" ? pth_write_png(temporal_path.c_str(), img.data(), W, H) : pth_write_ppm(temporal_path.c_str(), img.data(), W, H);
        }
        if (rc != 0) return die("write", pth_last_error());
    }
    if (!denoise_path.empty()) {   // guides of the pixel centres + the a-trous filter of the final accumulator, on the first context
        const size_t n_pix = (size_t)W * H;
        // with --temporal-out the history is filtered, not the last frame
        void *color = temporal ? t_color[1 - t_cur] : accum, *alb = nullptr, *nrm = nullptr, *pos = nullptr, *dout = nullptr, *drgba = nullptr;
        if (pt_malloc(ctx, n_pix * 16, &alb) != PT_OK || pt_malloc(ctx, n_pix * 16, &nrm) != PT_OK || pt_malloc(ctx, n_pix * 16, &pos) != PT_OK ||
            pt_malloc(ctx, n_pix * 12, &dout) != PT_OK || pt_malloc(ctx, n_pix * 4, &drgba) != PT_OK)
            return die("pt_malloc", pt_last_error(ctx));
        if (gpus > 1) {   // the stripes of the other contexts: the gathered frame, uploaded to a buffer of the first
            host_acc.resize(n_pix * 3);
            if (int grc = gather(accums, host_acc.data(), 12)) return grc;
            if (pt_malloc(ctx, n_pix * 12, &color) != PT_OK || pt_upload(ctx, color, host_acc.data(), n_pix * 12) != PT_OK)
                return die("pt_upload", pt_last_error(ctx));
        }
        const pt_denoise_params dn = {W, H, 4, 0.0f, 1.0f, 0.03f};   // = gpu_pathtracer_amd.DENOISE_DEFAULTS
        if (pt_render_aux(ctx, &cam, &p, (float*)alb, (float*)nrm, (float*)pos, nullptr) != PT_OK) return die("pt_render_aux", pt_last_error(ctx));
        if (denoise_variance) {   // the luminance stop from the moments of the run; every pixel has constantPdf samples, no lengths
            void* mom = moments[0];
            if (gpus > 1) {
                host_mom.resize(n_pix * 2);
                if (int grc = gather(moments, host_mom.data(), 8)) return grc;
                if (pt_malloc(ctx, n_pix * 8, &mom) != PT_OK || pt_upload(ctx, mom, host_mom.data(), n_pix * 8) != PT_OK)
                    return die("pt_upload", pt_last_error(ctx));
            }
            // = gpu_pathtracer_amd.DENOISE_VARIANCE_DEFAULTS
            const pt_denoise_variance_params dv = {W, H, 4, 4.0f, 1.0f, 0.03f, (float)std::max<uint64_t>(constantPdf, 1), 0};
            if (pt_denoise_variance(ctx, &dv, (const float*)color, (const float*)mom, nullptr, (const float*)alb, (const float*)nrm,
                                    (const float*)pos, (float*)dout, nullptr, (uint32_t*)drgba) != PT_OK)
                return die("pt_denoise_variance", pt_last_error(ctx));
            if (pt_sync(ctx) != PT_OK) return die("pt_sync", pt_last_error(ctx));
            if (gpus > 1) pt_free(ctx, mom);
        } else if (pt_denoise(ctx, &dn, (const float*)color, (const float*)alb, (const float*)nrm, (const float*)pos, (float*)dout, (uint32_t*)drgba) != PT_OK)
            return die("pt_denoise", pt_last_error(ctx));
        const std::string ext = denoise_path.size() > 4 ? denoise_path.substr(denoise_path.size() - 4) : std::string();
        int rc;
        if (ext == ".pfm") {
            std::vector<float> img(n_pix * 3);
            if (pt_download(ctx, img.data(), dout, img.size() * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
            rc = pth_write_pfm(denoise_path.c_str(), img.data(), W, H);
        } else {
            std::vector<uint32_t> img(n_pix);
            if (display) {
                if (int drc = display_words(dout, img)) return drc;
            } else if (pt_download(ctx, img.data(), drgba, img.size() * 4) != PT_OK) return die("pt_download", pt_last_error(ctx));
            rc = ext == ".png" ? pth_write_png(denoise_path.c_str(), img.data(), W, H) : pth_write_ppm(denoise_path.c_str(), img.data(), W, H);
        }
        if (rc != 0) return die("write", pth_last_error());
        for (void* b : {alb, nrm, pos, dout, drgba}) pt_free(ctx, b);
        if (gpus > 1) pt_free(ctx, color);
    }
    if (temporal) {
        for (int k = 0; k < 2; k++)
            for (void* b : {t_color[k], t_len[k], t_alb[k], t_nrm[k], t_pos[k], t_id[k]})
                if (b) pt_free(ctx, b);
        pt_free(ctx, t_rgba);
    }
    for (int g = 0; g < gpus; g++)
        for (int b = 0; b < 2; b++)
            if (spin_buf[(size_t)g * 2 + b]) pt_free(ctxs[(size_t)g], spin_buf[(size_t)g * 2 + b]);
    if (eq_rays) pt_free(ctx, eq_rays);
    for (void* b : {tone_rgba, tone_state})
        if (b) pt_free(ctx, b);
    (void)accum; (void)rgba;
    if (moments_all != moments[0]) pt_free(ctx, moments_all);
    for (int g = 0; g < gpus; g++) {
        if (moments[(size_t)g]) pt_free(ctxs[(size_t)g], moments[(size_t)g]);
        pt_free(ctxs[(size_t)g], accums[(size_t)g]);
        pt_free(ctxs[(size_t)g], rgbas[(size_t)g]);
        pt_destroy(ctxs[(size_t)g]);
    }
    if (bvh) pth_bvh_free(bvh);
    pth_mesh_free(mesh);
    return 0;
}
