/*
 * ptmi.h — C ABI of the MI355X-native progressive path tracer ("libptmi.so").
 *
 * This is the drop-in boundary for the ONE host→device call of the reference:
 *
 *     void BasicScene::launchKernel(const kernelInfo&)
 *         declared  GpuPathTracer/BasicScene.hpp:32
 *         defined   GpuPathTracer/tracer.cu:405-415   (trace<<<grid,16x16>>>(info))
 *         called    GpuPathTracer/BasicScene.cpp:404   (once per displayed frame)
 *
 * plus the device-buffer set-up the reference's constructor performs for that call
 * (cudaMalloc/cudaMemcpy of the three CudaBVH arrays and the sphere array,
 * GpuPathTracer/BasicScene.cpp:138-149, :214-215, :297-313).
 *
 * Everything crossing the boundary is plain C: fixed-width integers, float arrays,
 * raw pointers and sizes.  No glm, no bool, no C++ default initialisers (kernelInfo,
 * GpuPathTracer/CpuStructs.hpp:45-72, is not a C layout), no torch types.
 *
 * Conventions
 *   - every function returns 0 on success and a negative pt_status on failure; nothing
 *     ever calls exit() (the reference's checkCudaErrors does: utilfun.hpp:81-90);
 *     pt_last_error(ctx) returns a human-readable message for the last failure.
 *   - a ctx binds one HIP device and one stream.  Calls on one ctx are not re-entrant;
 *     different ctxs may be driven from different threads / processes (one per GPU).
 *   - pt_render is asynchronous with respect to the host until pt_sync.
 *   - "device pointer" arguments may come from pt_malloc or from any other HIP
 *     allocator in the same process (hipMalloc, a torch tensor's data_ptr()).
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_ABI_VERSION 3

typedef struct pt_ctx pt_ctx;

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = -1,   /* bad argument (null pointer, zero size, inconsistent arrays) */
    PT_ERR_DEVICE = -2,    /* a HIP call failed (message has hipGetErrorString)           */
    PT_ERR_NO_SCENE = -3,  /* pt_render / pt_trace_rays before pt_upload_bvh              */
    PT_ERR_NOMEM = -4,
    PT_ERR_UNSUPPORTED = -5
} pt_status;

/* Mat, GpuPathTracer/CommomStructs.hpp:12 — same numeric values. */
enum { PT_MAT_DIFF = 0, PT_MAT_METAL = 1, PT_MAT_SPEC = 2, PT_MAT_REFR = 3 };

/* pt_params.flags */
enum {
    /* METAL lobe adds float(image width)*cos(theta) to every component, exactly as
     * tracer.cu:280 does (`w` there is the int image width from tracer.cu:45).
     * Default (flag clear) is the intended  w1*cos(theta)  (SURVEY.md §3.4 table). */
    PT_FLAG_METAL_LITERAL_W = 1u << 0,
    /* also write the 0x00BBGGRR display word (tracer.cu:394-398); needs rgba_dev. */
    PT_FLAG_WRITE_RGBA = 1u << 1,
    /* Corrected-estimator switches — EXTENSIONS, all off by default so that the default path is the
     * reference's arithmetic, quirks included.  Oracle: same flags. */
    PT_FLAG_FACE_FORWARD = 1u << 2,  /* triangles: nl = dot(n,d) < 0 ? n : -n — what tracer.cu:126-127
                                        computes and then discards (nl = n in the reference)           */
    PT_FLAG_COSINE_DIFF = 1u << 3,   /* DIFF lobe: cosine-weighted direction from TWO draws (smallpt's
                                        estimator; mask *= col is then exact) instead of the reference's
                                        lobe, which draws sin(theta) uniformly in [0, 1] (density
                                        cos(theta) / (2 pi sin(theta)) per steradian about the normal, no
                                        weight), and its two discarded draws (tracer.cu:159-186)       */
    PT_FLAG_GLASS_FIX = 1u << 4,     /* REFR: R0 = ((nt-nc)/(nt+nc))^2 (the reference's :230 multiplies
                                        where it should divide), reflection chosen with probability
                                        P = .25 + .5 Re (the weights RP/TP assume it; the reference
                                        uses 0.2), transmitted rays start on the far side (-nl)       */
    PT_FLAG_RUSSIAN_ROULETTE = 1u << 5,/* from the 3rd segment on: continue with probability
                                        p = max(col) and divide col by p, else end the path          */
    PT_FLAG_RR_CPU_TRACER = 1u << 7,   /* Russian roulette exactly as the reference's CPU tracer plays it
                                        (CpuRayTracer/src/scene.cpp:38-47): from the 6th hit of a path on, continue
                                        with probability 0.9 p, p = max(col), and scale col by 0.9 / p — an expected
                                        0.81 per bounce: that renderer's energy loss, reproduced so that its images
                                        can be matched; PT_FLAG_RUSSIAN_ROULETTE is the unbiased one            */
    PT_FLAG_NEE = 1u << 8,             /* next-event estimation at DIFF hits (needs PT_FLAG_COSINE_DIFF): one shadow ray towards
                                        ONE of the emissive spheres the hit point is outside of (of the first 8 spheres;
                                        picked uniformly, cone-sampled, weighted by their number), and a DIFF-sampled ray
                                        that then lands on such a sphere does not count its emission again.  With a material
                                        table on the context (pt_upload_tri_materials) the TRIANGLES whose row emits are
                                        lights too: the pick is uniform over eligible spheres + emissive triangles, a point
                                        is drawn uniformly on the triangle (the faces a path can hit emit: the front one
                                        under cull_backfaces, both otherwise), and the next DIFF-sampled hit on any emissive triangle is not counted again.
                                        Spheres the path is inside of (the reference room's glowing walls) and triangles
                                        lit by the one global material of pt_params are gathered by the bounce as before.
                                        Same expectation, less noise for small lights; runs in the stage-split pipeline
                                        (a shadow-ray stage per bounce) or the megakernel.  An environment map uploaded
                                        under PT_OPT_ENV_LIGHT is one more light of the pick where the call also has
                                        PT_FLAG_MISS_KEEPS_PATH (the environment section states the rule)                    */
    PT_FLAG_MIS = 1u << 9,             /* multiple importance sampling under PT_FLAG_NEE (needs it: PT_ERR_INVALID without): at a
                                        DIFF hit that is not the path's last the shadow ray and the bounce ray are weighed
                                        against each other by the balance heuristic, per light, instead of the bounce ray
                                        dropping what the shadow ray could have picked.  Same draws, same expectation; less
                                        noise where one of the two samples badly (a large emitter close by, a small sun in a
                                        map).  "Multiple importance sampling" below states it.  Runs PT_KERNEL_MEGA_BVH2
                                        whatever PT_OPT_KERNEL says (no PT_KERNEL_AUTO trial; its table is neither read nor
                                        changed); PT_ERR_UNSUPPORTED over Woop records (PT_OPT_TRI_TEST 1)                   */
    PT_FLAG_MISS_KEEPS_PATH = 1u << 6 /* a segment that hits nothing ends the path with
                                        accu + mask * bk_color (smallpt, and the reference's own CPU
                                        tracer: CpuRayTracer/src/scene.cpp:27 returns black for the
                                        MISSING TERM only) instead of the reference GPU kernel's bare
                                        bk_color, which throws the gathered light away
                                        (tracer.cu:140-142)                                          */
};
/* The estimator of the reference's CPU tracer (CpuRayTracer/src/scene.cpp:23-56, material.cpp:24-45: smallpt's):
 * cosine-weighted diffuse lobe, normals facing the ray, Russian roulette, light only where a path ENDS on
 * emission.  With bk_color = 0, an emitter given col = 0 and a generous depth the expected radiance equals
 * that renderer's (tests/test_reference_radiance.py compares them). */
#define PT_FLAGS_SMALLPT (PT_FLAG_FACE_FORWARD | PT_FLAG_COSINE_DIFF | PT_FLAG_RUSSIAN_ROULETTE | PT_FLAG_MISS_KEEPS_PATH)
/* ... and with that renderer's own roulette instead of the unbiased one: its images, bias included */
#define PT_FLAGS_CPU_TRACER (PT_FLAG_FACE_FORWARD | PT_FLAG_COSINE_DIFF | PT_FLAG_RR_CPU_TRACER | PT_FLAG_MISS_KEEPS_PATH)

/* pt_ctx kernel selection (pt_set_option PT_OPT_KERNEL).  The values 2 and 4 of ABI 1-2 (a reserved name and the
 * round-1 role-split experiment) are gone with ABI 3: pt_set_option rejects them with PT_ERR_UNSUPPORTED. */
enum {
    PT_KERNEL_AUTO = 0,      /* PT_KERNEL_PERSISTENT or PT_KERNEL_WAVEFRONT, whichever is faster for the
                                configuration (image, samples per call, depth, partition shape, scene, material and
                                material table, environment map, flags): the first four pt_render calls of a configuration are timed trials, two per
                                layout (HIP events; buffers are allocated before the timed span; the faster trial
                                of each layout counts) and the following ones run the faster; the images are the same.  The decision never blocks the
                                host: while a trial's events are still pending, calls run the persistent kernel.
                                The library remembers the last 8 configurations.  pt_auto_choice reports it   */
    PT_KERNEL_MEGA_BVH2 = 1, /* one lane per pixel, one wave per 8x8 tile, bounce by bounce      */
    PT_KERNEL_PERSISTENT = 3,/* persistent waves: work queue, ballot/prefix-count lane refill    */
    PT_KERNEL_WAVEFRONT = 5  /* stage split (BASELINE.json configs[4]): path records in HBM, one
                                launch per stage — per bounce extend (persistent waves walking the
                                BVH, lanes refilled from the ray queue) and shade (one lane per
                                live path; survivors compacted with a ballot / prefix count into
                                the next generation).  Needs a BVH, depth >= 1 and the wide walk
                                over exact records; anything else runs PT_KERNEL_PERSISTENT.  Same images.
                                A context with an environment map (pt_upload_environment) is such a case:
                                this value and PT_KERNEL_AUTO (no trials) run PT_KERNEL_PERSISTENT, and with
                                PT_FLAG_NEE PT_KERNEL_MEGA_BVH2, until the map is cleared                  */
};

enum {
    PT_OPT_KERNEL = 1,        /* one of PT_KERNEL_*                                        */
    PT_OPT_COUNTERS = 2,      /* 1 = instrumented launch: fill pt_counters (slower)         */
    PT_OPT_TIMING = 3,        /* 1 = bracket every launch with hipEvents (pt_last_kernel_ms) */
    PT_OPT_BATCH = 4,         /* persistent kernel: waiting lanes (1..64) that make a wave
                                 leave the traversal loop to shade / refill; default 36      */
    PT_OPT_TOP_NODES = 5,     /* BVH nodes (breadth-first prefix, 0..1024) mirrored in LDS    */
    PT_OPT_OCCUPANCY = 6,     /* waves per SIMD the registers are budgeted for: 4/5/6/8 (default 6) */
    PT_OPT_LDS_STACK = 7,     /* traversal-stack entries kept in LDS per lane: 16 (default), 24 or
                                 0 = all 72; deeper entries overflow to private memory        */
    PT_OPT_WALK = 8,          /* closest-hit walk: 0 = while-while (Aila-Laine order, as the
                                 reference), 1 = unified-step over the binary tree,
                                 2 (default) = wide: unified-step over a 4-way tree with
                                 8-bit outward-rounded boxes; 4 = wide with one postponed leaf
                                 per lane (persistent kernel; the megakernel runs walk 2): a few
                                 per cent faster at 5 waves/SIMD, level at 8; all report the
                                 same hits                                                      */
    PT_OPT_REFILL = 11,       /* persistent kernel: idle lanes (1..64) that trigger a refill from the
                                 work queue; default 8; values above PT_OPT_BATCH are
                                 clamped to it (a wave must always have work to go to)          */
    PT_OPT_VOTE_NODE = 12,    /* walk 4: a wave runs a node step when                              */
    PT_OPT_VOTE_REC = 13,     /*   lanes_with_node * VOTE_NODE >= lanes_with_record * VOTE_REC (1, 1) */
    PT_OPT_WAVE_BATCH = 14,   /* PT_KERNEL_WAVEFRONT, extend stage: finished lanes (1..64) that make a wave leave the
                                 walk to store their hits and take new rays from the queue; default 16 */
    PT_OPT_SPHERE_LDS = 15,   /* persistent kernel: 1 (default) = the shading code reads the spheres from an LDS
                                 copy instead of scalar / global loads                            */
    PT_OPT_WAVE_BLOCKS = 19,  /* PT_KERNEL_WAVEFRONT, extend stage: resident 256-thread blocks per CU its persistent grid is
                                 sized for, 1..8 (default 8 = 8 waves per SIMD); fewer leave room for another
                                 context's launches on the same device                                 */
    PT_OPT_WAVE_SAMPLES = 25, /* PT_KERNEL_WAVEFRONT, bounce 0: how many samples of ONE pixel share a wave — the largest power of two
                                 <= this value (4 .. 64) that divides the call's spp; 16 by default (a wave = 16 samples x a 2x2
                                 pixel block: the samples of a pixel are the same ray but for the sub-pixel jitter, so they walk the
                                 same nodes and records in step), 1 = one sample of a whole 8x8 tile per wave as in the other
                                 kernels.  A speed knob: which lane traces which (pixel, sample) changes no result       */
    PT_OPT_FIRST_WALK = 26,   /* PT_KERNEL_WAVEFRONT, extend of bounce 0: 1 (default) = wave-wide packets — a wave walks ONE node or
                                 leaf at a time for the lanes whose own box tests lead there, fetching it once with scalar loads;
                                 0 = every lane walks on its own, as at the later bounces.  Same closest hits, hence the same
                                 images.  The packet walk keeps a stack of (link, lane mask) per wave in LDS; a tree that needs more
                                 than PT_OPT_PACKET_STACK entries (3 x wide depth + 2) runs the per-lane walk.  Woop records
                                 (PT_OPT_TRI_TEST 1) never reach this stage: they run PT_KERNEL_PERSISTENT              */
    PT_OPT_PACKET_STACK = 27, /* PT_OPT_FIRST_WALK 1: the packet stack's budget in entries per wave, 2..72 (default 72); a smaller
                                 value only sends deeper trees to the per-lane walk                                      */
    PT_OPT_OVERLAP = 21,      /* 1 (default): the path kernel of a pt_render call (persistent / mega kernels) runs on a
                                 stream of the context's own, so that it can start while the PREVIOUS call's last paths
                                 drain; the fold into the accumulator stays on the caller's stream, in call order.  When
                                 the caller's stream is idle at the call — a host that syncs before every launch, as
                                 BasicScene.cpp:395 does — the call runs in line on the caller's stream instead;
                                 0 = always in line                                                             */
    PT_OPT_BUILD_ALGO = 16,   /* pt_build_bvh: 1 (default) = PLOC (locally-ordered clustering over Morton order:
                                 a tree as good as the host SAH/SBVH builder's, ~6.5 ms for 800 k triangles;
                                 degenerate input falls back to 0), 0 = LBVH (Karras hierarchy: 1.8 ms, a
                                 tree that traces ~14 % slower)                                    */
    PT_OPT_REBUILD = 17,      /* pt_upload_bvh: 1 = keep the uploaded TRIANGLES but build the hierarchy again on
                                 the device (PT_OPT_BUILD_ALGO).  Same closest hits, hence the same images, except
                                 where a ray GRAZES a bounding plane: the binary32 slab test is not watertight, so
                                 a hit whose box is missed by one rounding in one tree and kept in the other can
                                 differ (measured: 2 of 2 073 600 pixels of the 16-spp 800k-triangle bench frame;
                                 every such pixel is arbitrated against brute force in tests/test_gpu_wide.py).
                                 Faster or slower than the caller's tree depending on the scene.
                                 2 = build it as well and keep whichever 4-wide tree has the smaller area cost
                                 in node visits (pt_tree_cost: the term that tracks the measured frame time,
                                 DESIGN.md 5.5) — the caller's on architectural scenes with long triangles
                                 that its spatial splits cut, the re-clustered one on dense scans; costs one
                                 device build (7 ms for 800 k triangles) per upload.  Default 0           */
    PT_OPT_OPTIMIZE = 24,     /* pt_upload_bvh / pt_build_bvh: 0 (default) = walk the hierarchy as it comes (after PT_OPT_LEAF_MAX); n > 0 = n
                                 passes of insertion-based optimisation over it first (Bittner et al. 2013: every node is taken out
                                 and re-inserted where the tree's surface-area cost grows least; csrc/pt_tree_opt.h) — on the host's
                                 threads, ~0.2 s per pass and million nodes on 64 threads; three passes get nearly all there is.  Same
                                 closest hits (grazing cases as PT_OPT_REBUILD).  A device-built tree (pt_build_bvh, PT_OPT_REBUILD)
                                 is fetched back, optimised and installed again.  cornell_dragon_800k: area cost in node visits /
                                 bench step, host SBVH tree 14.4 / 9.65 ms -> 12.6 / 9.00; host SAH tree without spatial splits
                                 14.6 / 9.95 -> 11.7 / 8.87; the device's PLOC tree 12.75 / 9.26 -> 12.1 / 9.15.  With
                                 PT_OPT_REBUILD 2 the two optimised hierarchies compete                                         */
    PT_OPT_PRESPLIT = 18,     /* pt_build_bvh / PT_OPT_REBUILD: 0 (default) = off; v > 0 = triangles longer than
                                 v per cent of (scene diagonal / sqrt(n triangles)) enter the builder as up
                                 to 8 primitives, one per slab of their box (early split clipping)      */
    PT_OPT_TRI_TEST = 10,     /* triangle records built at the next pt_upload_bvh: 0 = v0/e1/e2
                                 for Moller-Trumbore, what the reference kernel runs
                                 (cudaUtils.h:135-172; default, bit-exact vs the oracle);
                                 1 = Woop affine rows (north_star; CudaBVH.cpp:274-305 done
                                 right), tolerance-class parity, wide walk only.  Tolerance-class
                                 parity: the triangle a ray reports agrees with exact geometry
                                 outside the margins tests/woop_ref.py derives from the test's
                                 rounding steps (du = 6 * 2^-24 * (|rx.w| + sum |o_i rx_i| +
                                 |t| sum |d_i rx_i|) + t's own error); dyadic axis-plane geometry
                                 (unit axis edges, integer translations) is exact.  The margin
                                 grows with |v2| / edge length (the cancellation in rx.w +
                                 dot(o, rx)): measured median du 2.2e-5 on bunny_low at the
                                 origin, 1.7e-2 moved by (2^10, -2^12, 2^8)        */
    PT_OPT_LEAF_MAX = 9,      /* leaves holding more triangle references than this are split
                                 at the next pt_upload_bvh (0 = keep the producer's leaves;
                                 default 2)                                                   */
    PT_OPT_FUSE_STAGES = 28,  /* PT_KERNEL_WAVEFRONT without PT_FLAG_NEE or PT_OPT_COUNTERS: 1 (default) = bounce 0 is shaded in
                                 the launch of its packet walk (no hit records of bounce 0), and when every region of the call holds
                                 all samples of its pixels (PT_OPT_WAVE_SAMPLES groups of spp = 16, 8 or 4, depth >= 2) the last
                                 shade launch folds them into the accumulator (no separate fold launch); 0 = one launch per
                                 stage.  Same images, same counters                                                     */
    PT_OPT_LAST_ANYHIT = 29,  /* PT_KERNEL_WAVEFRONT: after `depth` segments only the gathered light is returned, so a path's last
                                 segment matters only through the emission of what it ends on.  When no triangle can emit (tri_emi
                                 all zero, no pt_upload_tri_materials table; also depth >= 2, no PT_FLAG_NEE, at most 8 spheres,
                                 PT_OPT_TRI_TEST 0) the shade launch before it records the nearest sphere hit ts of the new ray, and
                                 the last walk only answers "is a triangle hit at t <= ts?", leaving at the first such record
                                 instead of finding the closest one.  1 (default) = product launches do so; 2 = instrumented
                                 (PT_OPT_COUNTERS) launches too: pt_get_counters then counts the shorter walk and
                                 pt_get_wave_stats [5] the rays of that launch (0 = it did not run); 0 = closest hit on every
                                 segment.  With 0 or 1 the counters are those of the closest-hit walk.  Same images            */
    PT_OPT_ROOT_CULL = 30,    /* PT_KERNEL_WAVEFRONT: a surviving path's new ray that the walk's own first node step would turn away
                                 at the tree's root (no child box of the 4-wide root entered before t_max: the ray misses the mesh, or
                                 enters it beyond the sphere bound of PT_OPT_LAST_ANYHIT) is not queued for the next extend launch.
                                 The shade lane that made the ray runs that node step itself, packs such records behind the region's
                                 walkers and writes the hit record of a miss for them.  1 (default) = product launches do so; 2 =
                                 instrumented (PT_OPT_COUNTERS) launches too: pt_get_counters then lacks one node visit per such ray
                                 (`rays` still counts them) and pt_get_wave_stats [10] is their number; 0 = every survivor is
                                 queued.  With 0 or 1 the counters are those of the full queue.  Same images                     */
    PT_OPT_ROOT_ENTRY = 33,   /* PT_KERNEL_WAVEFRONT with PT_OPT_ROOT_CULL: the shade lane keeps the rest of that node step as well —
                                 which of the root's four children the new ray enters, nearest first — as an 8-bit code in the
                                 record's sample word, and the extend launches of the later bounces start every walk behind the
                                 root: the far children on the stack, the nearest one as the first item, without fetching or testing
                                 the root again.  Needs PT_OPT_ROOT_CULL on for the call, no PT_FLAG_NEE and spp < 4096 (the sample
                                 number gives up eight bits); any other call keeps the plain record and walks from the root, with
                                 every limit unchanged.  1 (default) = product launches do so; 2 = instrumented (PT_OPT_COUNTERS)
                                 launches too (with PT_OPT_ROOT_CULL 2): pt_get_counters then lacks one more node visit per ray the
                                 extend launches of bounces >= 1 drew (pt_get_wave_stats [7] is their number while bounce 0 is the
                                 packet walk, PT_OPT_FIRST_WALK 1); 0 = every walk starts at the root.
                                 With 0 or 1 the counters are unchanged.  Same images                                           */
    PT_OPT_PATH_HISTORY = 34, /* PT_KERNEL_WAVEFRONT: a path's record carries WHICH objects the path has hit so far — four bits per
                                 bounce, sphere 0-7 or "a triangle" — in one word instead of its mask as three floats; a shade lane
                                 rebuilds the mask and the light gathered so far from that word with the arithmetic the path itself
                                 would have done, and the path's sample colour is written once, by the lane the path ends in, not
                                 added to at every bounce.  Holds for calls whose mask and gathered light depend on nothing else: no
                                 PT_FLAG_NEE, PT_FLAG_RUSSIAN_ROULETTE or PT_FLAG_RR_CPU_TRACER, no per-triangle materials, at most
                                 8 spheres, no PT_MAT_REFR triangle material or sphere, depth <= 9; any other call keeps the three
                                 mask planes and the in-place adds.  1 (default) = product launches do so; 2 = instrumented
                                 (PT_OPT_COUNTERS) launches too; 0 = off.  No counter changes under any value.  Same images         */
    PT_OPT_ENV_LIGHT = 35,    /* read by the next pt_upload_environment: 0 (default) = the map is what a miss gathers and nothing
                                 else; 1 = the map also gets a sampling distribution and is a LIGHT under PT_FLAG_NEE (see the
                                 environment section).  Any other value PT_ERR_INVALID                                            */
    PT_OPT_LAST_OCCLUDERS = 36 /* PT_KERNEL_WAVEFRONT with PT_OPT_LAST_ANYHIT and PT_OPT_ROOT_CULL on for the call: the last segment
                                 only asks whether SOME triangle lies at t <= ts, so the shade lane that makes the ray first tests it
                                 against the mesh's largest triangles (pt_occluder_ids: the walls of a room), read from a small table
                                 with scalar loads, with the walk's own test on the walk's own records.  A ray one of them occludes is
                                 packed with the rays the root turns away and gets the verdict the any-hit walk would have written;
                                 it is never queued.  A mesh without such triangles has no list and runs the launches it ran before.
                                 pt_refit_bvh copies the listed triangles' moved records on its stream.  1 (default) = product
                                 launches do so; 2 = instrumented (PT_OPT_COUNTERS) launches too (with PT_OPT_LAST_ANYHIT 2 and
                                 PT_OPT_ROOT_CULL 2): `rays` still counts those rays, pt_get_wave_stats [11] is their number, [5] and
                                 `inner`, `tris`, `leaves` lack their walks; 0 = off.  With 0 or 1 the counters are unchanged.
                                 Same images                                                                                    */
};

/* CamInfo, GpuPathTracer/CpuStructs.hpp:19-28 (pitch/yaw/dirty/bias/enabled are host-only
 * GUI state and never read by the kernel: cudaUtils.h:111-134). */
typedef struct pt_camera {
    float pos[3];
    float front[3];
    float right[3];
    float up[3];
    float dist;
    float aspect;
    float fov;
    float _pad;
} pt_camera;

/* Sphere, GpuPathTracer/CommomStructs.hpp:18-39 — 44 bytes, same field order. */
typedef struct pt_sphere {
    float pos_rad[4];  /* centre xyz, radius */
    float emi[3];
    float col[3];
    int32_t mat;       /* PT_MAT_* */
} pt_sphere;

/* The scalar part of kernelInfo (GpuPathTracer/CpuStructs.hpp:45-72) that the kernel
 * reads (tracer.cu:27-400); pointer members travel as explicit arguments. */
typedef struct pt_params {
    int32_t width, height;        /* kernelInfo::width/height                              */
    uint32_t depth;               /* kernelInfo::depth          (tracer.cu:72)             */
    int32_t cull_backfaces;       /* kernelInfo::cullBackFaces  (cudaUtils.h:151-155)      */
    uint64_t frame;               /* frameNumber; the kernel seed is uf::hash(frame)
                                     (BasicScene.cpp:397, utilfun.cpp:380-389)             */
    uint64_t sample_index;        /* kernelInfo::constantPdf = N of the running mean for
                                     the first sample of this call; 1 = overwrite
                                     (BasicScene.cpp:399, tracer.cu:386-391)               */
    int32_t tri_mat;              /* kernelInfo::triCurrentMat  (tracer.cu:135)            */
    float tri_col[3];             /* kernelInfo::col            (tracer.cu:131)            */
    float tri_emi[3];             /* kernelInfo::emi            (tracer.cu:132)            */
    float bk_color[3];            /* kernelInfo::bkColor        (tracer.cu:141)            */
    float air_ior;                /* kernelInfo::air_ref_index                              */
    float glass_ior;              /* kernelInfo::glass_ref_index                            */
    float phong_expo;             /* kernelInfo::phongExpo                                  */
    uint32_t flags;               /* PT_FLAG_*                                              */
    /* Framebuffer partition for multi-GPU tile split (new; the reference is single-GPU).
     * The image is cut into stripes of `part_rows` rows; this call renders only stripes
     * s with  s % part_count == part_index.  part_count <= 1 renders everything.
     * RNG is keyed by the GLOBAL pixel index, so any partition gives bit-identical
     * pixels.  accum/rgba are always full-frame buffers. */
    int32_t part_index, part_count, part_rows;
    int32_t _pad;
} pt_params;

/* Work counters of the last instrumented launch (PT_OPT_COUNTERS=1).  They are the
 * N_* of the algorithmic-byte definition in SURVEY.md §8(d). */
typedef struct pt_counters {
    uint64_t rays;        /* closest-hit queries (ray segments)          */
    uint64_t inner;       /* inner nodes fetched                          */
    uint64_t tris;        /* triangle records tested                      */
    uint64_t leaves;      /* leaves entered                               */
    uint64_t hits;        /* segments that ended on a triangle            */
    uint64_t paths;       /* pixel-samples                                */
} pt_counters;

/* ---- context ------------------------------------------------------------------ */
int pt_abi_version(void);
int pt_device_count(void);                       /* <0 on error                     */
int pt_create(int device, pt_ctx** out);
int pt_destroy(pt_ctx* ctx);
const char* pt_last_error(const pt_ctx* ctx);     /* ctx may be NULL: global message  */
/* pt_set_stream: the stream the following calls are issued on; NULL = the ctx's own.  A switch in the middle of a session needs no
 * pt_sync: the new stream waits (on the device, an event) for everything the old one has been given — the context's scratch buffers, its
 * light list and a refit tree are shared by the calls on either — so the calls of one ctx keep their order across the switch.  The old
 * stream must still exist at the switch. */
int pt_set_stream(pt_ctx* ctx, void* hip_stream);
int pt_set_option(pt_ctx* ctx, int option, int value);
int pt_sync(pt_ctx* ctx);

/* ---- memory (thin; callers may also pass pointers from their own allocator) ----- */
int pt_malloc(pt_ctx* ctx, size_t bytes, void** dev_out);
int pt_free(pt_ctx* ctx, void* dev);
int pt_memset(pt_ctx* ctx, void* dev, int value, size_t bytes);
int pt_download(pt_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int pt_upload(pt_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);

/* ---- scene -------------------------------------------------------------------
 * pt_upload_bvh consumes the three host arrays CudaBVH::createCompact produces
 * (GpuPathTracer/CudaBVH.cpp:121-270) — exactly what BasicScene.cpp:297-306 copies:
 *   nodes      getGpuNodes()/getGpuNodesSize():  vec4[n_node_vec4], 4 per inner node,
 *              child link >=0 = BYTE offset of the child node, <0 = ~(first tri vec4)
 *   tri_verts  getDebugTri()/getDebugTriSize():  vec4[n_tri_vec4], per leaf
 *              {v0,v1,v2 (xyz,0)}*k followed by one 0x80000000 terminator vec4
 *   tri_index  getGpuTriIndices():               int[n_index], parallel to tri_verts
 * The arrays are validated, copied and re-laid-out for gfx950; the host
 * arrays may be freed when the call returns. */
int pt_upload_bvh(pt_ctx* ctx,
                  const float* nodes, size_t n_node_vec4,
                  const float* tri_verts, size_t n_tri_vec4,
                  const int32_t* tri_index, size_t n_index);
int pt_upload_spheres(pt_ctx* ctx, const pt_sphere* spheres, size_t n_spheres);

/* Build the acceleration structure ON THE DEVICE from an indexed triangle mesh — an EXTENSION
 * (the reference builds on the host: SplitBVHBuilder.cpp, BasicScene.cpp:281-294).
 * Morton order + PLOC clustering (or the Karras linear BVH, PT_OPT_BUILD_ALGO) collapsed into the
 * same item buffer pt_upload_bvh produces, in milliseconds; the PLOC tree traces as fast as the host
 * SAH/SBVH builder's.  Rendered images equal those over an uploaded hierarchy except for rays that graze a
 * bounding plane (see PT_OPT_REBUILD: a handful of pixels per 2 M at 800 k triangles, none on the small
 * scenes of the test suite).  Triangle ids are the row numbers of `tris`.  PT_OPT_LEAF_MAX (default 2)
 * = triangles per leaf.  verts: float[n_verts][3], tris: int32[n_tris][3]; host arrays, copied.
 * PT_ERR_INVALID: a coordinate that is not finite or has |x| > 3.0e38, or a mesh whose extent max - min on an axis is not a finite
 * binary32 (-2e38 beside +2e38: the 4-wide node's grid step is extent / 255, pt_items.h).  pt_refit_bvh cannot refuse: its caller
 * keeps the moved mesh within that extent.  pt_upload_bvh takes the caller's boxes as they are (the same limit holds for them). */
int pt_build_bvh(pt_ctx* ctx, const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris);
int pt_last_build_ms(pt_ctx* ctx, float* ms_out);   /* device time of the build behind the tree on the context (pt_build_bvh or a
                                                       kept PT_OPT_REBUILD tree); PT_ERR_INVALID for an uploaded hierarchy */

/* Move the triangles of the scene on the context — an EXTENSION (an update / refit operation): the hierarchy keeps its
 * topology and every box is refit on the device, so an optimised tree (PT_OPT_OPTIMIZE, PT_OPT_REBUILD) survives animation.
 * tri_verts_dev: float[n_tris][9] = v0, v1, v2 of the triangle whose ORIGINAL id is the row (the ids of the Compact index
 * array, or the rows of pt_build_bvh's `tris`); device memory (pt_malloc, hipMalloc, a torch tensor).  n_tris must cover
 * every id of the tree; rows the tree does not reference are ignored.
 * A triangle with a coordinate that is not finite or has |x| > 3.0e38 (pt_build_bvh's rule) is dropped: it is never hit and
 * adds nothing to any box.  When n_dropped_dev != NULL, the number of dropped triangles is written there (uint32, device).
 * Boxes are the min / max of the three vertices, as pt_build_bvh computes them: a refit to the vertices a device tree was
 * built from reproduces that tree bit for bit.  A spatial-split reference (host SBVH, PT_OPT_PRESPLIT) gets its whole
 * triangle's box: correct, but looser.  Woop records (PT_OPT_TRI_TEST 1): PT_ERR_UNSUPPORTED.
 * Asynchronous on the context's stream.  It is ordered after earlier pt_render / pt_trace_rays calls and before later ones,
 * side streams (PT_OPT_OVERLAP) included.  The first refit of a tree synchronises once: it reads the tree's shape back (links,
 * ids and leaf flags: 8 bytes per binary node and per record, 16 per wide node) and allocates and uploads the per-height
 * schedule and scratch boxes, about 24 bytes per record + 40 per binary and per wide node of device memory, held until the
 * tree is replaced or the context destroyed and not counted in pt_scene_info.  Later refits neither allocate nor synchronise.
 * With PT_OPT_TIMING=1, pt_last_kernel_ms reports the refit's device time.  pt_scene_info, pt_last_build_ms and the tree's
 * generation are unchanged.  Every tree this library installs has an inner root (pt_build_bvh doubles a lone triangle); a
 * tree without the [binary nodes][records][wide nodes] layout would give PT_ERR_UNSUPPORTED. */
int pt_refit_bvh(pt_ctx* ctx, const float* tri_verts_dev, size_t n_tris, uint32_t* n_dropped_dev);
/* The occluder list pt_upload_bvh and pt_build_bvh choose for a mesh (PT_OPT_LAST_OCCLUDERS), host only, no context: the triangles
 * whose area (half |e1 x e2|, binary64 from the binary32 vertices) is at least 1/24 of the mesh's (summed in id order), largest first,
 * equal areas by the smaller id, at most min(cap, 12).  Writes their ids to ids_out and returns their number (0: no list, as for a
 * mesh without walls); PT_ERR_INVALID for a NULL array, a negative cap or an index >= n_verts.  pt_upload_bvh applies the rule to the
 * distinct triangle ids of its Compact arrays. */
int pt_occluder_ids(const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris, int32_t* ids_out, int cap);

/* Per-triangle materials — an EXTENSION.  The reference parses the .mtl into
 * `materials` but never reads it (utilfun.cpp:458-462) and shades every triangle with the ONE
 * material of kernelInfo (tracer.cu:131-135 = pt_params.tri_mat/tri_col/tri_emi/phong_expo).
 * After this call a triangle with ORIGINAL id i (the ids of the Compact index array) is shaded
 * with table[tri_material[i]] instead; everything else of the path loop is unchanged.
 * n_materials = 0 clears the table (back to the reference's behaviour).  n_tris must cover
 * every id of the uploaded BVH.  Arrays are copied. */
typedef struct pt_material {
    float col[3];        /* albedo (mask *= col)                 */
    float emi[3];        /* emitted radiance (accu += mask*emi)  */
    int32_t mat;         /* PT_MAT_*                             */
    float phong_expo;    /* METAL lobe exponent                  */
} pt_material;           /* 32 bytes */
int pt_upload_tri_materials(pt_ctx* ctx, const pt_material* table, size_t n_materials,
                            const int32_t* tri_material, size_t n_tris);

/* ---- the hot path -------------------------------------------------------------
 * render(accum, bvh, camera, spp) of BASELINE.json: fold `spp` consecutive samples
 * (frames params->frame .. frame+spp-1, running-mean N = sample_index .. +spp-1) into
 * accum_dev (float[height][width][3], the reference's vec3 accumBuffer) and, when
 * PT_FLAG_WRITE_RGBA is set, the display word into rgba_dev (uint32[height][width],
 * the reference's dev_drawRes).  Equals `spp` single-sample calls bit for bit. */
int pt_render(pt_ctx* ctx, float* accum_dev, uint32_t* rgba_dev,
              const pt_camera* cam, const pt_params* params, uint32_t spp);

/* pt_render that also keeps the luminance moments of its samples — an EXTENSION: what an error-driven stop,
 * adaptive sampling or a variance-aware filter start from (the accumulator is a CLAMPED running mean, so its own history does
 * not say how noisy a pixel is).  moments_dev: float[height][width][2] = (m1, m2), device memory, 8-byte aligned.
 * moments_dev == NULL: exactly pt_render.  Otherwise the accumulator and the display words are what pt_render writes, bit for
 * bit, and for every pixel the call owns (part_* as for the accumulator) and every sample s of the call in order, with
 * N = sample_index + s and col the sample colour BEFORE the fold's clamp:
 *     L  = (0.2126f * col.x + 0.7152f * col.y) + 0.0722f * col.z        plain * and +, every step one binary32 rounding
 *     m1 = N == 1 ? L     : (m1 * (float)(N - 1) + L)     * (1.0f / (float)N)
 *     m2 = N == 1 ? L * L : (m2 * (float)(N - 1) + L * L) * (1.0f / (float)N)
 * No clamp (a firefly shows in m2) and no fused multiply-add, so that binary32 arithmetic anywhere restates it exactly.
 * N == 1 overwrites, as for the accumulator: the moments continue across calls, and spp samples in one call equal any split of
 * them over several calls bit for bit.  Pixels the call does not own are not touched.  Errors, flags, materials, partitions and
 * every PT_OPT_* as pt_render; the moments depend on them only through the sample colours.  The moments are kept by the fold
 * launch over the call's sample buffer, so such a call always has one: a one-sample call of the persistent / mega kernels does
 * not fold in line, and the stage-split pipeline keeps its separate fold launch (PT_OPT_FUSE_STAGES fuses bounce 0 only).
 * PT_KERNEL_AUTO decides for calls with and without moments separately. */
int pt_render_moments(pt_ctx* ctx, float* accum_dev, uint32_t* rgba_dev, float* moments_dev,
                      const pt_camera* cam, const pt_params* params, uint32_t spp);

/* One error figure for a frame from its moments after n_samples samples per pixel.  Per pixel, in binary32:
 *     var = max(0, m2 - m1 * m1),   rse = sqrtf(var / (float)(n_samples - 1)) / (m1 + 0.01f)
 * — the relative standard error of the mean luminance; 0.01 is a floor that keeps a black pixel at 0 instead of 0 / 0 (a
 * definition, not a tuned value).  *mean_rse = sum of rse over all width x height pixels / their number (summed in double per
 * 256-pixel block on the device, the blocks added on the host in order: the same figure run after run); *n_above = pixels with
 * rse > threshold.  Either output may be NULL, not both.  moments_dev: float[height][width][2], device memory.
 * PT_ERR_INVALID: NULL ctx / moments / both outputs, width or height < 1, n_samples < 2, a threshold that is not finite or is
 * negative.  No scene needed.  Synchronises the context's stream (hence ordered after the folds of earlier calls).  Its scratch
 * (12 bytes per 256 pixels) belongs to the context: grown on demand, freed by pt_destroy. */
int pt_frame_error(pt_ctx* ctx, const float* moments_dev, int32_t width, int32_t height,
                   uint64_t n_samples, float threshold, double* mean_rse, uint64_t* n_above);

/* Closest-hit query on an explicit ray batch (rows a5–a7 of SURVEY.md §8 in isolation,
 * = intersectBVHandTriangles, cudaUtils.h:256-460).  rays_dev: float[n][8] =
 * (ox,oy,oz,tmin=0, dx,dy,dz,unused); out t_dev float[n] (F32_MAX on miss),
 * tri_dev int32[n] (original triangle id, -1 on miss), normal_dev float[n][3]
 * (un-normalised cross(v0-v1, v0-v2) of the winner; may be NULL). */
int pt_trace_rays(pt_ctx* ctx, const float* rays_dev, size_t n_rays, int cull_backfaces,
                  float* t_dev, int32_t* tri_dev, float* normal_dev);

/* ---- bounded ray-batch queries — an EXTENSION ---------------------------
 * pt_closest_hits and pt_any_hits answer "what does this ray hit" and "is this segment blocked" for a caller's rays: shadow and
 * visibility tests, ambient occlusion, picking, line of sight.  Both run the 4-wide walk of the stage-split pipeline's extend
 * stage on persistent waves (a tree too deep for that walk takes the binary walk of pt_trace_rays and gives the same results).
 *   rays_dev: float[n][8] = (ox, oy, oz, ignored, dx, dy, dz, t_max) — pt_trace_rays' stride; word 3 is never read.
 * A triangle is hit when 0 < t < t_max in binary32, strict on both sides, with t from the records and the arithmetic of
 * pt_trace_rays (cull_backfaces included).  t_max = +inf or any value >= FLT_MAX: unbounded.  A ray whose t_max is not greater
 * than 0 (0, negative, NaN) is a miss and is not walked.  Triangles only: the spheres take no part, as in pt_trace_rays.
 * The walk prunes boxes with the bound too, and a box's entry distance is not rounded as a triangle's t is; so that a hit just
 * below t_max is not lost with its box, every ray's box tests (never its triangle tests) are widened by a margin above the
 * rounding error of both: t_max = the next float above a hit's t finds the hit, t_max = t does not.
 *   pt_closest_hits, for the nearest such hit (of two at the same t the smaller id): t_dev float[n] (FLT_MAX on a miss, not the
 *     bound), tri_dev int32[n] (original id, -1 on a miss), normal_dev float[n][3] as pt_trace_rays writes it (0 on a miss; may
 *     be NULL).  With t_max = +inf these are pt_trace_rays' outputs, except that a grazing ray may pass between the two trees'
 *     boxes differently (see PT_OPT_REBUILD).
 *   pt_any_hits: hit_dev uint8[n], 1 when such a hit exists, else 0; one byte per ray and nothing beyond byte n - 1 (the
 *     storage of a torch.bool tensor qualifies).
 * The outputs must not overlap rays_dev (a lane reads rays that another lane's result could already have overwritten); this is
 * not checked.  Errors, in this order: NULL ctx PT_ERR_INVALID; no tree PT_ERR_NO_SCENE; Woop records (PT_OPT_TRI_TEST 1)
 * PT_ERR_UNSUPPORTED; n_rays == 0 PT_OK, nothing written; a NULL rays_dev, t_dev, tri_dev or hit_dev PT_ERR_INVALID;
 * n_rays >= 2^32 PT_ERR_INVALID.  Asynchronous on the context's stream: ordered after pt_refit_bvh, usable between pt_render
 * calls, and no call allocates or synchronises (the work counters belong to the context and are reset on the stream before
 * each launch).  With PT_OPT_TIMING=1, pt_last_kernel_ms covers the call.  PT_OPT_WAVE_BATCH, PT_OPT_WAVE_BLOCKS and
 * PT_OPT_LDS_STACK 24 apply as to the extend stage: speed, never results.  PT_OPT_COUNTERS is ignored (pt_get_counters keeps
 * the last render's figures).  Left out: a t_min other than 0, spheres, Woop records, per-ray cull flags, which triangle an
 * any-hit query found. */
int pt_closest_hits(pt_ctx* ctx, const float* rays_dev, size_t n_rays, int cull_backfaces,
                    float* t_dev, int32_t* tri_dev, float* normal_dev);
int pt_any_hits(pt_ctx* ctx, const float* rays_dev, size_t n_rays, int cull_backfaces,
                uint8_t* hit_dev);

/* ---- radiance along a caller's rays — an EXTENSION -----------------------
 * pt_render_rays path-traces rays the caller made: other cameras (fisheye, equirectangular, orthographic, thin lens, stereo),
 * light probes, baking, paths continued from a host's own visibility pass.  pt_render derives a path's first segment from the pinhole
 * camera and the pixel; here it is read from a buffer, and everything behind it is the path kernels' loop unchanged: depth,
 * cull_backfaces, spheres, the global or per-triangle materials, every PT_FLAG_* estimator switch, next-event estimation, roulette.
 *   rays_dev: float[n][8] = (ox, oy, oz, ignored, dx, dy, dz, ignored) — pt_trace_rays' stride; words 3 and 7 are never read.  d is
 *     used as given, NOT normalised: pass unit directions, as pt_render's camera makes them (the spheres' test and every lobe
 *     assume them).
 *   radiance_dev: float[n][3], the running mean per ray; must not overlap rays_dev (not checked).
 * Ray i, sample s = 0 .. spp-1: a path that starts at (o, d) with the random stream of pt_render's pixel number first_index + i in
 * frame params->frame + s, positioned behind the two draws a camera path spends on its sub-pixel jitter.  So a batch equal to a
 * camera's rays of frame f (jitter included), with first_index = 0, width = the image's and frame = f, reproduces that frame's
 * samples bit for bit.  All spp samples of a ray start from the same ray; a caller who wants anti-aliasing jitters its rays
 * across calls.  The samples are folded in order with N = params->sample_index + s, N == 1 overwrites:
 *   PT_RAYS_CLAMPED  pt_render's fold exactly: a = clamp01((a * (N - 1) + col) * (1 / N)) per component;
 *   PT_RAYS_HDR      a = (a * (N - 1) + col) * (1 / N), no clamp, plain binary32 * and + (a = 0 in front of the sum when N == 1):
 *                    for probes and baking.
 * spp samples in one call equal any split of them over several calls (frame and sample_index advanced alike) bit for bit, and one
 * call over n rays equals calls over its parts with first_index advanced by the rays before each part: first_index splits a batch
 * over calls or contexts.
 * pt_params: depth, cull_backfaces, frame, sample_index, tri_mat / tri_col / tri_emi, bk_color, air_ior, glass_ior, phong_expo and
 * flags are read as by pt_render; width only by PT_FLAG_METAL_LITERAL_W; height, part_* and PT_FLAG_WRITE_RGBA are ignored.
 * depth == 0 folds black samples, as pt_render does.
 * A ray whose direction has a component that is not finite or is (0, 0, 0), or whose origin is not finite, is never walked or
 * tested against a sphere: its samples are those of a path whose first segment hit nothing — bk_color (under
 * PT_FLAG_MISS_KEEPS_PATH the same value as 0 + 1 * bk_color), also when the context has an environment map
 * (pt_upload_environment): there is no direction to look up; at depth 0 black like every other ray.
 * Errors, in this order: NULL ctx PT_ERR_INVALID; neither a tree nor spheres PT_ERR_NO_SCENE; n_rays == 0 or spp == 0 PT_OK,
 * nothing written; a NULL rays_dev, radiance_dev or params PT_ERR_INVALID; a mode other than the two PT_ERR_INVALID;
 * n_rays >= 2^32 PT_ERR_INVALID; then pt_render's own: sample_index == 0, a bad tri_mat, PT_FLAG_NEE without PT_FLAG_COSINE_DIFF,
 * then PT_FLAG_MIS without PT_FLAG_NEE,
 * PT_ERR_INVALID; PT_FLAG_NEE over emissive triangles, or PT_FLAG_MIS, with Woop records PT_ERR_UNSUPPORTED.  Woop records (PT_OPT_TRI_TEST 1)
 * otherwise run, as in pt_render's persistent kernel: the wide walk with tolerance-class parity, PT_ERR_UNSUPPORTED when the tree is
 * too deep for that walk.
 * The kernel is the persistent kernel's loop — (sample, ray) slots drawn from a work queue by resident waves, the 4-wide walk, or
 * the binary one for PT_OPT_WALK 0 / 1 and for trees too deep — so a few rays with many samples fill the device as well as many
 * rays with one.  PT_OPT_BATCH, PT_OPT_REFILL and PT_OPT_SPHERE_LDS apply: speed, never results.  PT_OPT_KERNEL, PT_OPT_COUNTERS and
 * PT_KERNEL_AUTO's table are neither read nor changed (pt_get_counters keeps the last render's figures).
 * Asynchronous on the context's stream: ordered after pt_refit_bvh, usable between pt_render calls.  With spp > 1 the samples go
 * through the context's sample buffer ([spp][n][3] floats, at most 768 MiB: more samples run as several launches), which pt_render
 * shares: grown on demand — that call synchronises the stream once — freed by pt_destroy, not counted in pt_scene_info.  With
 * PT_OPT_TIMING=1, pt_last_kernel_ms covers the call.
 * Left out: the stage-split pipeline and its packet walk for ray batches; a per-ray t_max or t_min; per-ray RNG keys other than
 * first_index + i; luminance moments; display words. */
enum { PT_RAYS_CLAMPED = 0, PT_RAYS_HDR = 1 };
int pt_render_rays(pt_ctx* ctx, const float* rays_dev, size_t n_rays, uint64_t first_index,
                   float* radiance_dev, const pt_params* params, uint32_t spp, int mode);

/* ---- camera models: the rays pt_render_rays reads, made on the device — an EXTENSION ------------
 * pt_camera_rays writes, for frame `frame`, the jittered ray of every pixel of an image (or of a listed subset) under one of five
 * camera models straight into a buffer of pt_render_rays' layout: no host loop, no upload, no pt_sync in between.  One call per
 * sample gives anti-aliasing, and depth of field under PT_CAM_THIN_LENS, which needs a fresh ray per sample.
 * Row i is the ray of pixel pix = pixels_dev ? pixels_dev[i] : first_pixel + i, px = pix % width, py = pix / width, written as
 * (o.xyz, 0, d.xyz, 0): pt_trace_rays' stride, words 3 and 7 always 0.  rays_dev: float[n][8], 16-byte aligned.
 * Jitter: the random stream of pt_render's pixel number pix in frame `frame` (csrc/pt_math.h: pt_rng_init of pt_wang64 [frame] and
 * pix), jx = next - 0.5f, jy = next - 0.5f — the two draws and the arithmetic with which pt_render's camera path starts, the two
 * draws pt_render_rays' stream stands behind.  So for PT_CAM_PINHOLE, this call for frame f over all pixels, then pt_render_rays
 * with first_index 0, frame f, spp 1 and sample_index N, folds the sample pt_render folds for frame f, bit for bit.  With
 * PT_CAMF_CENTRE jx = jy = 0 and nothing is drawn.
 * Lens draws (PT_CAM_THIN_LENS only): (v0, v1) are the first two draws of a SECOND stream, that of pixel pix in "frame"
 * frame ^ PT_CAM_LENS_KEY — draws 2 onward of the first stream belong to the path.
 * The models.  front, right, up, pos, dist, aspect, fov are pt_camera's; W, H = width, height.  binary32 throughout, plain * and +
 * but for the fused operations of vdot(u, v) = fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x)), normalize(v) = v * (1 / sqrtf(vdot(v, v)))
 * and v * s + w = fmaf per component where a point or direction is built from the basis.  The basis is used as given; every model
 * but the pinhole assumes it orthonormal.  ax = ((px - W/2) + 0.5) + jx, ay = ((py - H/2) + 0.5) + jy: the pixel's offsets from
 * the image centre as pt_render's camera forms them.
 *   PT_CAM_PINHOLE    pt_render's camera ray (getCamRayDir, cudaUtils.h:111-134): dir0 = front * dist + right * xs + up * ys with
 *                     xs = ax * dist * aspect * fov / (W - 1), ys = ay * dist * fov / (H - 1); o = pos + dir0 — the reference's
 *                     origin ON the image plane and its division by W - 1 — and d = normalize(dir0).  The one model pinned bit
 *                     for bit (against pt_render and the oracle).
 *   PT_CAM_THIN_LENS  dir0 as above; the point in focus pf = pos + dir0 * (focus_dist / dist); the lens point
 *                     l = pos + right * (R r cos phi) + up * (R r sin phi), r = sqrtf(v0), phi = 2 pi v1 (the path kernels' sincos),
 *                     R = lens_radius; o = l, d = normalize(pf - l).  R = 0: o = pos exactly, d the pinhole's direction.
 *   PT_CAM_ORTHO      o = pos + right * (ax * ortho_height * aspect / W) + up * (ay * ortho_height / H), d = normalize(front).
 *   PT_CAM_FISHEYE    equidistant: Rpx = min(W, H) / 2, rho = sqrtf(ax * ax + ay * ay), theta = rho / Rpx * (fisheye_fov / 2);
 *                     o = pos, d = normalize(front * cos theta + (right * ax + up * ay) * (sin theta / rho)), d = normalize(front)
 *                     where rho == 0.  A pixel with theta > fisheye_fov / 2 lies outside the image circle and has no ray: its
 *                     row is o = pos, d = (0, 0, 0), which pt_render_rays renders as a miss (bk_color).
 *   PT_CAM_EQUIRECT   the layout of `pt_app --equirect` and of pt_upload_environment (an integer coordinate is a texel centre):
 *                     fx = px + jx, fy = py + jy, lon = (fx - W/2) * (2 pi / W), lat = clamp((fy - H/2) * (pi / H), -pi/2, pi/2);
 *                     o = pos, d = normalize((front * cos lon + right * sin lon) * cos lat + up * sin lat).
 * With a pixel list an index >= W * H gives the zero-direction row too (o = pos): the host cannot check a device list.
 * Errors, in this order; nothing is written on any of them, nor for n == 0: NULL ctx PT_ERR_INVALID; n == 0 PT_OK; then each
 * PT_ERR_INVALID: a NULL cam, cm or rays_dev; an unknown model or unknown flag bits; width or height < 2, or width * height >= 2^32;
 * n >= 2^32; without a list, first_pixel + n > width * height; the parameter of the chosen model that is not finite or out of its
 * range (lens_radius >= 0 and focus_dist > 0; ortho_height > 0; 0 < fisheye_fov <= 2 pi) — the parameters of other models are
 * ignored.  No scene, no scratch, no allocation, no synchronisation: asynchronous on the context's stream, hence ordered before the
 * pt_render_rays that follows.  With PT_OPT_TIMING=1, pt_last_kernel_ms covers it.
 * Left out: guide buffers for these cameras in this call (pt_render_aux stays pinhole; pt_render_aux_camera below makes them and
 * pt_temporal_camera carries them across frames); stereo pairs (a host calls twice); lens shapes other than
 * a disk; RNG keys for pt_render_rays by pixel instead of first_index + i (a listed subset renders with the keys of its row
 * numbers); the generator fused into the path kernel. */
enum { PT_CAM_PINHOLE = 0, PT_CAM_THIN_LENS = 1, PT_CAM_ORTHO = 2, PT_CAM_FISHEYE = 3, PT_CAM_EQUIRECT = 4 };
enum { PT_CAMF_CENTRE = 1 };           /* no sub-pixel jitter: jx = jy = 0 (guides, picking, tests) */
#define PT_CAM_LENS_KEY 0xC3A5C85C97CB3127ull   /* frame ^ this keys the lens stream; the top bit is set, so no frame number a host counts up to meets its own lens stream */
typedef struct pt_camera_model {
    int32_t model;                     /* PT_CAM_*                                                    */
    int32_t width, height;             /* the image the pixel numbers refer to; >= 2 each, w*h < 2^32 */
    int32_t flags;                     /* PT_CAMF_*                                                   */
    float lens_radius;                 /* THIN_LENS: aperture radius, >= 0                            */
    float focus_dist;                  /* THIN_LENS: distance along front of the plane in focus, > 0  */
    float ortho_height;                /* ORTHO: world height of the view volume, > 0                 */
    float fisheye_fov;                 /* FISHEYE: full angle across the image circle, radians, (0, 2 pi] */
} pt_camera_model;                     /* 32 bytes */
int pt_camera_rays(pt_ctx* ctx, const pt_camera* cam, const pt_camera_model* cm, uint64_t frame,
                   const uint32_t* pixels_dev /* may be NULL */, size_t n, uint64_t first_pixel,
                   float* rays_dev /* float[n][8] */);

/* ---- a camera model's frame in one call: each sample's ray made in the path kernel — an EXTENSION ----
 * pt_render_camera path-traces pixels of a cm->width x cm->height image under any of the five camera models without a ray buffer
 * and without a launch per sample: what the loop "per sample, pt_camera_rays then a one-sample pt_render_rays" computes, in one
 * call.  binary32 throughout, as stated for those two calls.
 * Pixel of a row: row i is pixel pix = pixels_dev ? pixels_dev[i] : first_pixel + i.  radiance_dev: float[n][3], the running mean
 * per row; pixels_dev: n pixel numbers on the device, or NULL.
 * Ray of a sample: sample s = 0 .. spp-1 of row i starts at exactly the row pt_camera_rays writes for pix in frame
 * params->frame + s — the model's arithmetic, the jitter stream, PT_CAMF_CENTRE, the lens stream frame ^ PT_CAM_LENS_KEY, and the
 * zero-direction row of a fisheye pixel outside the image circle or of a listed index >= W * H, which pt_render_rays' guard makes a
 * first-segment miss (bk_color).
 * The path's random stream is that of pixel pix — not of the row number — in frame params->frame + s, standing behind the two
 * jitter draws: pt_render's stream for that pixel.  Under PT_CAMF_CENTRE it stands behind them too, as in the loop.
 * Everything behind the first segment is pt_render_rays': depth, materials, spheres, every PT_FLAG_*, next-event estimation, MIS,
 * the environment map (lookup and light), Woop records, and the fold with N = params->sample_index + s under PT_RAYS_CLAMPED /
 * PT_RAYS_HDR.  spp samples in one call equal any split of them over calls (frame and sample_index advanced alike) bit for bit, and
 * one call equals calls over its parts by first_pixel.  pt_params is read as by pt_render_rays: width only under
 * PT_FLAG_METAL_LITERAL_W — the image is cm's.
 * Guarantees (tests/test_gpu_render_camera.py):
 *   (a) without a list the result equals, bit for bit, the loop over s of pt_camera_rays(frame + s, first_pixel) and
 *       pt_render_rays(first_index = first_pixel, frame + s, sample_index + s, spp 1), for all five models;
 *   (b) hence with PT_CAM_PINHOLE, first_pixel 0, n = W * H and PT_RAYS_CLAMPED it is pt_render's accumulator bit for bit;
 *   (c) with a list, row i equals row pixels_dev[i] of the full-frame call bit for bit: repeated indices repeat the value, an index
 *       past the image gives the miss sample (bk_color).  So any listed subset of pixels renders with the bits of the full frame.
 * Errors, in this order; nothing is written on any of them: NULL ctx PT_ERR_INVALID; neither a tree nor spheres PT_ERR_NO_SCENE;
 * n == 0 or spp == 0 PT_OK, nothing written; a NULL cam, cm, radiance_dev or params PT_ERR_INVALID; a mode other than the two
 * PT_ERR_INVALID; pt_camera_rays' checks of cm, n and first_pixel in its order and with its wording, prefixed pt_render_camera:;
 * then pt_render_rays' remaining ones: sample_index == 0, a bad tri_mat, the PT_FLAG_NEE / PT_FLAG_MIS combinations, its refusals
 * over Woop records.
 * Asynchronous on the context's stream.  Scratch is the shared sample buffer under pt_render_rays' rule: [spp][n][3] floats, at most
 * 2^26 slots per launch, more samples go out as several launches.  With PT_OPT_TIMING=1, pt_last_kernel_ms covers the call.
 * PT_OPT_BATCH, PT_OPT_REFILL and PT_OPT_SPHERE_LDS apply: speed, never results.  PT_OPT_KERNEL, the counters and PT_KERNEL_AUTO's
 * table are neither read nor changed.  The kernel is pt_render_rays' loop with another path start (csrc/pt_rays_loop.h); the model
 * is a value of the launch, not an instantiation.
 * Left out: luminance moments in this call (pt_render_pixels below keeps them, for these cameras too); display words; guide buffers
 * for these cameras in this call (pt_render_aux_camera below makes them); the stage-split pipeline. */
int pt_render_camera(pt_ctx* ctx, const pt_camera* cam, const pt_camera_model* cm,
                     const uint32_t* pixels_dev /* may be NULL */, size_t n, uint64_t first_pixel,
                     float* radiance_dev /* float[n][3] */, const pt_params* params, uint32_t spp, int mode);

/* ---- adaptive sampling: more samples only where the image is noisy — an EXTENSION --------------------------
 * Two calls and a loop the host writes: pt_render_pixels renders listed pixels into full-frame buffers, each pixel from its own
 * sample count on, and keeps the luminance moments; pt_select_pixels makes the list of the pixels whose error figure is still above
 * a threshold, on the device.  zero the counts; pt_render_pixels over every pixel; then pt_select_pixels, pt_render_pixels over the
 * list, until nothing is selected.  binary32, plain * and +, as stated for pt_render_moments and pt_frame_error.
 *
 * pt_render_pixels is pt_render_camera folded into full-frame buffers with a sample count per pixel.  The image is cm's,
 * W x H = cm->width x cm->height.  accum_dev: float[H*W][3]; moments_dev: float[H*W][2] = (m1, m2), 8-byte aligned, may be NULL;
 * counts_dev: uint32[H*W], the samples each pixel holds; pixels_dev: n pixel numbers on the device, or NULL: every pixel, row i is
 * pixel i and n must be W * H.
 * Samples: sample s = 0 .. spp-1 of listed pixel pix is exactly the sample pt_render_camera makes for pix in frame
 * params->frame + s — the same ray and the same random stream, which is the pixel's and not the row's.  The path kernel is
 * pt_render_camera's, with the caller's list; a call of more than 2^26 slots goes out as several launches, each followed by its fold.
 * Fold: row i is pixel pix = pixels_dev ? pixels_dev[i] : i.  A pix >= W * H is skipped: nothing is written anywhere for it.
 * Otherwise, with c = counts[pix] and, for every sample s of the call in order, N = c + 1 + s and col the sample colour:
 *     accum[pix]   = pt_render_rays' running mean under the mode: (a * (float)(N - 1) + col) * (1.0f / (float)N), clamped to 0..1
 *                    per step under PT_RAYS_CLAMPED, not under PT_RAYS_HDR; N == 1 overwrites
 *     moments[pix] = pt_render_moments' formula with this N: L from col before the clamp, N == 1 overwrites, no fused multiply-add
 * and then counts[pix] = c + spp.  N == 1 overwrites, so only counts_dev needs zeroing before the first pass.
 * params->sample_index must be >= 1, as for every path call, and is otherwise not read: the counts carry N.
 * A pixel listed twice in one call is the caller's error: it is not checked and the result for that pixel is unspecified.  A count
 * that would pass 2^32 - 1 is the caller's error too.
 * Guarantees (tests/test_gpu_adaptive.py):
 *   (a) with pixels_dev == NULL, n == W * H and all counts equal to k, accum equals pt_render_camera's full-frame result with
 *       sample_index = k + 1 bit for bit, for all five models and both modes; hence with PT_CAM_PINHOLE and PT_RAYS_CLAMPED it is
 *       pt_render's accumulator, and in that case moments equals pt_render_moments';
 *   (b) with a list, a listed pixel gets what (a) gives it for its own count, and every unlisted pixel keeps its bits in all three
 *       buffers;
 *   (c) any split of spp over calls, frame advanced alike, gives the same bits: the counts carry N;
 *   (d) so a host loop whose pass k renders frames params->frame + k * pass_spp .. + pass_spp - 1 and whose selection only ever
 *       drops pixels leaves every pixel with count c the accumulator and moments of pt_render_moments(spp = c) at params->frame.
 * Errors: pt_render_camera's, in its order, prefixed pt_render_pixels: — NULL ctx; no scene; n == 0 or spp == 0 PT_OK, nothing
 * written; a NULL cam, cm, accum_dev, counts_dev or params; the mode; the model, its flags, the image, n >= 2^32; without a list an
 * n other than W * H PT_ERR_INVALID; the model's parameter; sample_index == 0, a bad tri_mat, the PT_FLAG_NEE / PT_FLAG_MIS
 * combinations, the refusals over Woop records.
 * Asynchronous on the context's stream.  Scratch is the shared sample buffer, [min(spp, 2^26 / n)][n][3] floats and always used,
 * also at spp == 1: the moments and the counts are the fold's job, as for pt_render_moments.  With PT_OPT_TIMING=1,
 * pt_last_kernel_ms covers the call and pt_get_stage_ms splits it into the path launches (PT_STAGE_FRAME) and the folds (PT_STAGE_FOLD).
 * Options as for pt_render_camera.
 * Left out: display words; a sample count read on the device for the path launch (the host passes n). */
int pt_render_pixels(pt_ctx* ctx, const pt_camera* cam, const pt_camera_model* cm,
                     const uint32_t* pixels_dev /* may be NULL: every pixel */, size_t n,
                     float* accum_dev /* float[H*W][3] */, float* moments_dev /* float[H*W][2]; may be NULL */,
                     uint32_t* counts_dev /* uint32[H*W] */, const pt_params* params, uint32_t spp, int mode);

/* pt_select_pixels: the pixels that need more samples, as an ascending list made on the device.  Per pixel, in binary32, with
 * n = counts[pix] and (m1, m2) = moments[pix]:
 *     n >= 2:  var = fmaxf(0, m2 - m1 * m1),   rse = sqrtf(var / (float)(n - 1)) / (m1 + 0.01f)      pt_frame_error's, with the pixel's own n
 *     n <  2:  rse = 0
 *     an rse that is not finite counts as 0 and is never selected (a NaN pixel would be rendered again for ever)
 *     selected  <=>  n < max_samples  and  (n < max(min_samples, 2)  or  rse > threshold)               (strictly above)
 * pixels_dev[0 .. *n_selected) receives the selected pixel numbers in ASCENDING order — neighbouring pixels land in neighbouring
 * lanes of the path kernel, and the list is the same run after run; nothing is written beyond entry *n_selected - 1.  pixels_dev:
 * uint32[W*H].  *mean_rse (may be NULL) = the sum of rse over all pixels / (W * H), summed in double over pt_frame_error's 256-pixel
 * blocks with its reduction tree, the blocks added on the host in order: for uniform counts n it equals pt_frame_error(.., n, ..)'s
 * figure exactly, and with min_samples = 0 and max_samples = UINT32_MAX *n_selected equals its n_above.
 * Three launches over 256-pixel blocks (count, one block's exclusive scan of the counts, write at the rank): no block waits for
 * another and nothing is added atomically.  The call then copies the blocks' sums and counts back and SYNCHRONISES the context's
 * stream, like pt_frame_error: one synchronisation per adaptive pass.  Scratch, 16 bytes per block, belongs to the context: grown
 * on demand, freed by pt_destroy.  No scene needed.
 * Errors, in this order, PT_ERR_INVALID each: NULL ctx; a NULL sp, moments_dev, counts_dev, pixels_dev or n_selected; width or
 * height < 1, or W * H >= 2^32; a threshold that is not finite or is negative; min_samples > max_samples.
 * Note: selecting by the variance of the same samples that form the mean is biased — a pixel that looks converged by chance stops
 * early, and dark pixels are under-sampled.  min_samples is the guard.
 * Left out: the unbiased scheme with two sample buffers (one to decide, one to show); a sample count for the path launch that
 * stays on the device. */
typedef struct pt_select_params {
    int32_t width, height;
    float threshold;                    /* finite, >= 0 */
    uint32_t min_samples, max_samples;  /* min <= max */
    int32_t _pad;
} pt_select_params;                     /* 24 bytes */
int pt_select_pixels(pt_ctx* ctx, const pt_select_params* sp, const float* moments_dev, const uint32_t* counts_dev,
                     uint32_t* pixels_dev /* uint32[W*H] */, uint64_t* n_selected, double* mean_rse /* may be NULL */);

/* ---- environment map — an EXTENSION -----------------------------------------
 * pt_upload_environment gives the context a latitude-longitude (equirectangular) radiance map: what a path segment that hits
 * nothing gathers instead of the one constant bk_color, so that open scenes — a mesh on its own, a probe rendered elsewhere — are
 * lit by an image.  The layout is the one `pt_app --equirect` writes: with (front, right, up) the frame the map is laid out in,
 * column x looks at longitude (x - W/2) 2 pi / W from `front` towards `right`, row y at latitude (y - H/2) pi / H towards `up`.
 *   texels: host float[height][width][3], copied; the device copy is float4[height][width] = (r, g, b, 0) with `scale` folded in
 *   (texel * scale, one binary32 rounding), so a lookup is one or four 16-byte gathers.
 * The lookup of a direction d (any length; pt_render_rays' directions need not be unit for it), in binary32 with plain * and +,
 * the only fused operations those of vdot(u, v) = fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x)), in this order:
 *   1. a = vdot(d, front), b = vdot(d, right), c = vdot(d, up); one of them not finite, or all three 0: the result is (0, 0, 0).
 *   2. lon = atan2f(b, a), lat = atan2f(c, sqrtf(a * a + b * b)).
 *   3. fx = lon * kx + hx, fy = lat * ky + hy with kx = W / 2 pi, ky = H / pi, hx = W / 2, hy = H / 2, each computed in double and
 *      rounded once.  An integer (fx, fy) is a texel.
 *   4. PT_ENV_NEAREST: column floorf(fx + 0.5f) wrapped into 0..W-1, row floorf(fy + 0.5f) clamped into 0..H-1.
 *   5. PT_ENV_BILINEAR: x0 = floorf(fx), wx = fx - x0, columns x0 and x0 + 1 wrapped; y0 = floorf(fy), wy = fy - y0, rows y0 and
 *      y0 + 1 clamped; per component lerp(p, q, w) = p + w * (q - p), the columns within each row first, then the two rows — so
 *      a constant map returns its constant exactly.
 * Where it applies: in pt_render, pt_render_moments and pt_render_rays a segment that hits neither a triangle nor a sphere returns
 * the lookup of its direction where it returned bk_color, by the same rule of the flags — the bare value, or accu + mask * value
 * under PT_FLAG_MISS_KEEPS_PATH (the reference's quirk that a miss without that flag is NOT masked holds for a map too).  Every
 * flag, partitions and PT_FLAG_NEE work; under NEE the map is gathered by bounce rays only, like a sphere the path is inside of —
 * unless it was uploaded under PT_OPT_ENV_LIGHT (below), a map with a small sun is noisy.  pt_render_rays' guard keeps writing bk_color for a ray that
 * is not finite or has no direction (there is nothing to look up).  pt_render_aux, pt_denoise and pt_temporal are untouched: a
 * pixel that sees the map is still a miss.  With a map on the context the stage-split pipeline is not chosen (see
 * PT_KERNEL_WAVEFRONT); clearing the map brings it back.  A map change is a scene change for PT_KERNEL_AUTO's table.
 * env == NULL clears the map: every call then behaves exactly as before, bk_color included.
 * The call waits for the context's streams, the side streams of PT_OPT_OVERLAP included, before it replaces or frees texels: a
 * render in flight reads the old map to its end, a render issued after the call reads the new one without the caller syncing.
 * The memory belongs to the context: freed by pt_destroy or a clear, not counted in pt_scene_info.
 * Errors, in this order: NULL ctx PT_ERR_INVALID; then with env != NULL, each PT_ERR_INVALID: a NULL texels; a dimension out of
 * range; an unknown filter; a basis vector or scale that is not finite, a zero basis vector, a negative scale (these four before
 * texels is dereferenced); a texel that is not finite or is negative after scaling.  The old map stays in place on any error.
 * Left out: the stage-split pipeline for scenes with a map, mip levels, cube or octahedral layouts, the map in pt_render_aux's
 * albedo.
 *
 * The map as a light.  A map carries a sampling distribution when PT_OPT_ENV_LIGHT was 1 at its upload, its
 * basis is orthonormal (in double: |len(v) - 1| <= 1e-4 for front, right and up, |dot| <= 1e-4 for each pair — the draw's inverse
 * mapping assumes it) and it is not black (T > 0 below); otherwise the upload succeeds as before and the map is no light.
 * pt_environment_is_light tells which.  The tables, built on the host in double, t the scaled device texel, every sum sequential
 * in ascending index:
 *   m[y][x] = max(t.r, t.g, t.b); for PT_ENV_BILINEAR the maximum of that over the 3 x 3 neighbourhood, columns wrapped and rows
 *     clamped, so that the density is positive wherever a bilinear lookup can be.
 *   Row edges by the lookup's nearest rule (row 0 owns fy in [0, 0.5), row H - 1 owns [H - 1.5, H]): e_0 = -pi/2,
 *     e_i = (i - 0.5 - H/2) * pi / H for 0 < i < H, e_H = +pi/2; zs[i] = (float)sin(e_i), zs[0] = -1 and zs[H] = 1 exactly.
 *   S_y = sum_x m[y][x]; cx[y][i] = (float)(sum_{j<i} m[y][j] / S_y) for i = 0..W, cx[y][0] = 0 and cx[y][W] = 1 exactly; a row
 *     with S_y = 0 gets i / W and is never picked.
 *   A_y = S_y * ((double)zs[y+1] - (double)zs[y]), T = sum A_y; cy[i] = (float)(sum_{j<i} A_j / T), cy[0] = 0, cy[H] = 1 exactly.
 * On the device float cx[H][W+1], cy[H+1], zs[H+1]: about 4 bytes per texel more, owned and freed with the map, not counted in
 * pt_scene_info; "the old map stays in place on any error" covers them.
 * The draw for (u1, u2) in [0, 1), binary32 with plain * and +:
 *   y = the largest i in 0..H-1 with cy[i] <= u1 (binary search: a zero-width row is never picked), py = cy[y+1] - cy[y],
 *     v1 = min((u1 - cy[y]) / py, 0x1.fffffep-1f); the same in row y with u2: x, px, v2.
 *   z = zs[y] + v1 * (zs[y+1] - zs[y]), r = sqrtf(max(0, 1 - z * z)), lon = ((((float)x - 0.5f) + v2) - hx) / kx,
 *     d = front * (r * cosf(lon)) + right * (r * sinf(lon)) + up * z.
 *   pdf = ((py * px) * kx) / (zs[y+1] - zs[y]) per steradian, constant over the texel — from the CDF DIFFERENCES, not m / T, so it is
 *     the density of what is drawn whatever the rounding of the tables; 0 where py * px is 0.
 *   (u1 = 0 in row 0, or v1 rounding to the far edge of row H - 1, is a pole itself: r = 0, where the columns of the row meet and the
 *   lookup of d takes longitude atan2f(0, 0) = 0, column W / 2, whatever column was drawn.)
 * The density of a given direction: a, b, c, fx, fy as in the lookup, column and row the lookup's nearest ones, the same formula;
 * 0 for a direction the lookup calls invalid.
 * The estimator: in pt_render, pt_render_moments and pt_render_rays, at a DIFF hit of a call with PT_FLAG_NEE,
 * PT_FLAG_COSINE_DIFF and PT_FLAG_MISS_KEEPS_PATH that is not the path's last (hit number `depth`: the bounce ray from there is
 * never traced, so what the map sends there lies beyond the call's depth and the call's expectation is the same with and without
 * the tables), such a map is the LAST light of PT_FLAG_NEE's uniform pick (n_all = eligible spheres + emissive triangles + 1); the draws are unchanged: u0 picks the light, u1 the row, u2 the column.  The shadow ray leaves
 * the hit point along d with no far end; it is dropped when dot(nl, d) <= 0, when pdf is not > 0 or when ANY sphere is hit at
 * ts > 0.01 (a point inside one of the room's wall spheres never sees the sky, as its bounce ray would not), else traced against
 * the triangles, and adds mask * lookup(d) * (cosl * n_all / (pi * pdf)) — the lookup the call renders with, either filter.  The
 * bounce ray of such a hit gathers nothing from the map when it leaves the scene (accu + mask * 0): the exclusive scheme the
 * spheres and emissive triangles use.  Camera rays, mirror / glass / metal bounces and calls without the three flags gather the
 * map as before; a context whose map is no light renders exactly what it rendered.
 * Left out: mip or hierarchical warps, building the tables on the device, the stage-split
 * pipeline with a map, the map as a light without PT_FLAG_MISS_KEEPS_PATH (a miss then discards the gathered light).
 *
 * Multiple importance sampling (PT_FLAG_MIS; pt_render, pt_render_moments, pt_render_rays).  binary32, plain * and
 * +.  The draws of PT_FLAG_NEE are unchanged (u0 picks the light, u1 and u2 draw on it): a path consumes the same random numbers
 * with and without the flag.  With pi = 3.14159274f, 2 pi = 6.28318548f:
 * At a DIFF hit x that is not the path's last (hit number < depth) and has n_all > 0 pickable lights, the shadow ray's contribution
 * is multiplied by w_l = q / (q + p_b), where p_b = cosl / pi is the cosine lobe's density of the drawn direction l and
 * q = p_k(l) / n_all the density with which the shadow ray draws it, p_k per steradian:
 *     sphere              1 / (2 pi (1 - cos_max)), cos_max as the cone draw computes it
 *     emissive triangle   2 d2 / proj, d2 the squared distance to the drawn point, proj = abs(dot(cross(e1, e2), l))
 *     environment map     the draw's pdf
 * Both weights are computed through r = n_all / p_k = 1 / q — n_all * (2 pi * (1 - cos_max)), n_all * (proj / (2 * d2)),
 * n_all / pdf — which stays finite where a light's solid angle rounds to 0:  w_l = 1 / (1 + p_b * r).
 * The path carries nee_mask (which lights were pickable at x) and p_b' = max(0, dot(nl, d)) / pi, the lobe's density of the bounce
 * direction d it takes, to its next vertex.  Where plain NEE drops the emission of what d hits, or the map's radiance when d leaves
 * the scene, because the light was pickable, it is added with w_b = p_b' / (p_b' + q') instead: a = min(p_b' * r', FLT_MAX),
 * w_b = a / (a + 1), r' = n_all / p_k(d) for the light that was hit, seen from the bounce ray's origin (the point the draws used),
 * n_all rebuilt from nee_mask (the sphere bits, + the emissive triangles, + 1 for the map):
 *     sphere i            the same cos_max arithmetic from the ray's origin: r' = n_all * (2 pi * (1 - cos_max))
 *     any triangle        r' = n_all * (abs(dot(N, d)) / (2 * (t * t))), N the hit's un-normalised normal (|N| = 2 area), t the
 *                         hit distance (a row that does not emit adds nothing whatever its weight)
 *     the map, on a miss  r' = n_all / pdf(d), "the density of a given direction" above; w_b = 1 where pdf(d) is not > 0
 * so that w_l + w_b = 1 for one direction seen from both sides.  Everything plain NEE gathers in full stays so: spheres the path
 * is inside of, spheres past the first 8, triangles under the one global material, whatever a mirror, glass or metal bounce
 * reaches (it clears nee_mask), camera rays.  At the path's last hit no bounce ray follows: the shadow ray keeps weight 1 and the map
 * is no light there, as under plain NEE — a depth-1 call renders the same bits with and without the flag, and the expectation at
 * every depth is plain NEE's.
 * Left out: the stage-split pipeline (its path record has no word for p_b'), the power heuristic, one-sample MIS, MIS for the
 * Phong lobe of PT_MAT_METAL (its bounce gathers in full). */
enum { PT_ENV_NEAREST = 0, PT_ENV_BILINEAR = 1 };
typedef struct pt_environment {
    int32_t width, height;               /* texels: 1..16384 each, width * height <= 2^26 */
    float front[3], right[3], up[3];     /* the frame the map is laid out in (pt_app --equirect's cam.front / right / up) */
    float scale[3];                      /* rgb factor, folded into the texels at upload: texel * scale, one rounding */
    int32_t filter;                      /* PT_ENV_* */
    int32_t _pad;
} pt_environment;                        /* 64 bytes */
int pt_upload_environment(pt_ctx* ctx, const pt_environment* env, const float* texels /* host float[h][w][3] */);
/* The lookup above for a ray batch — "what does the sky send from here": rays_dev float[n][8], pt_trace_rays' stride, words 4-6
 * (the direction) read, the rest ignored; radiance_dev float[n][3], must not overlap rays_dev (not checked).  One thread per ray.
 * Errors, in this order: NULL ctx PT_ERR_INVALID; no map PT_ERR_NO_SCENE; n_rays == 0 PT_OK, nothing written; a NULL pointer
 * PT_ERR_INVALID; n_rays >= 2^32 PT_ERR_INVALID.  Asynchronous on the context's stream; with PT_OPT_TIMING=1, pt_last_kernel_ms
 * covers it. */
int pt_eval_environment(pt_ctx* ctx, const float* rays_dev, size_t n_rays, float* radiance_dev /* float[n][3] */);
/* *out = 1 when the context's map carries a sampling distribution (see "The map as a light"), 0 when it does not or there is no
 * map.  NULL ctx or out: PT_ERR_INVALID. */
int pt_environment_is_light(pt_ctx* ctx, int* out);
/* The draw and the density above for a batch, one thread per element.  pt_sample_environment: u_dev float[n][2] = (u1, u2), a
 * value outside [0, 1) or a NaN clamped into [0, 0x1.fffffep-1] (a NaN to 0); dir_pdf_dev float[n][4] = (d.xyz, pdf);
 * radiance_dev float[n][3], the lookup along d (what pt_eval_environment answers for it), may be NULL.  pt_environment_pdf:
 * rays_dev float[n][8], words 4-6 read (any length); pdf_dev float[n].  Buffers must not overlap (not checked).
 * Errors, in this order: NULL ctx PT_ERR_INVALID; no map PT_ERR_NO_SCENE; a map that is no light PT_ERR_UNSUPPORTED; n == 0 PT_OK,
 * nothing written; a NULL required pointer PT_ERR_INVALID; n >= 2^32 PT_ERR_INVALID.  Asynchronous on the context's stream; with
 * PT_OPT_TIMING=1, pt_last_kernel_ms covers them. */
int pt_sample_environment(pt_ctx* ctx, const float* u_dev, size_t n, float* dir_pdf_dev, float* radiance_dev);
int pt_environment_pdf(pt_ctx* ctx, const float* rays_dev, size_t n, float* pdf_dev);

/* ---- guide buffers and denoiser — an EXTENSION --------------------------
 * pt_render_aux: the first hit of ONE ray through every pixel centre (the camera ray of pt_render with zero jitter), for a
 * denoiser or for picking.  Triangles by the binary closest-hit walk of pt_trace_rays, then the spheres with the path kernels'
 * rule (t > 0.01 and closer than the triangle).  Device outputs, row-major [height][width]:
 *   albedo_dev   float[4]  (r, g, b, 0): the `col` of what was hit — the sphere's, the triangle's material row
 *                          (pt_upload_tri_materials) or params->tri_col; emission is ignored
 *   normal_dev   float[4]  (x, y, z, 0): unit geometric normal facing the ray (dot(n, d) < 0), triangles and spheres alike
 *   position_dev float[4]  (x, y, z, t): the hit point o + t d and the ray distance t
 *   id_dev       int32     original triangle id (>= 0), -2 - i for sphere i, -1 on a miss; may be NULL
 * A miss writes 0 to every component of the three float buffers: a pixel is a miss exactly when its normal is (0, 0, 0).
 * Reads width, height, cull_backfaces and tri_col of params only (always the full frame; partition fields and flags are
 * ignored).  PT_ERR_NO_SCENE without a BVH, PT_ERR_UNSUPPORTED over Woop records (PT_OPT_TRI_TEST 1), PT_ERR_INVALID for a
 * NULL required pointer or width / height < 1.  Asynchronous on the context's stream (ordered after pt_refit_bvh); with
 * PT_OPT_TIMING=1, pt_last_kernel_ms reports its device time. */
int pt_render_aux(pt_ctx* ctx, const pt_camera* cam, const pt_params* params,
                  float* albedo_dev, float* normal_dev, float* position_dev, int32_t* id_dev);

/* pt_denoise: edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of an accumulator, guided by pt_render_aux's
 * buffers.  With a'_p = albedo_p where albedo_p > 1e-3 per channel, else 1 (misses: 1), the colour is demodulated,
 * i0 = c / a', then iteration l = 0 .. iterations-1 (step s = 2^l) computes
 *     i(l+1)_p = sum_q w_pq i(l)_q / sum_q w_pq,   q = p + s (dx, dy), dx, dy in -2..2, inside the image,
 *     w_pq = h(dx) h(dy) exp(-|i_p - i_q|^2 / (sigma_color 2^-l)^2 - |n_p - n_q|^2 / sigma_normal^2
 *                             - |x_p - x_q|^2 / (sigma_position t_p)^2),   h = (1, 4, 6, 4, 1) / 16,
 * the normal and position terms only where both p and q are hits, w = 0 where exactly one of them is a miss, a term with
 * sigma <= 0 left out (t_p = position.w of p: sigma_position is a fraction of the distance).  out = clamp01(i(L) a').
 * iterations = 0 copies color to out bit for bit.
 *   color_dev float[h][w][3] (pt_render's accumulator layout, never written); out_dev the same layout and may alias color_dev;
 *   rgba_dev (may be NULL) receives the 0x00BBGGRR display word of out, as pt_render packs it.
 * PT_ERR_INVALID: NULL color / guide / out pointer, width or height < 1, iterations outside 0..10, a non-finite sigma.  No
 * scene needed.  Asynchronous on the context's stream, hence ordered after the fold of an earlier pt_render (which stays on
 * that stream under PT_OPT_OVERLAP).  Scratch (two float[4] frames) belongs to the context: allocated on first use or when the
 * frame grows (that call synchronises once), freed by pt_destroy, not counted in pt_scene_info; a later call at the same or a
 * smaller size neither allocates nor synchronises.  With PT_OPT_TIMING=1, pt_last_kernel_ms covers all of its launches. */
typedef struct pt_denoise_params {
    int32_t width, height;
    int32_t iterations;                               /* 0..10                           */
    float sigma_color, sigma_normal, sigma_position;  /* <= 0 switches that term off     */
} pt_denoise_params;                                  /* 24 bytes                        */
int pt_denoise(pt_ctx* ctx, const pt_denoise_params* dp, const float* color_dev,
               const float* albedo_dev, const float* normal_dev, const float* position_dev,
               float* out_dev, uint32_t* rgba_dev);

/* pt_denoise_variance: pt_denoise's filter with its colour stop replaced by a LUMINANCE stop that each pixel scales by the
 * standard error of its own mean (the variance-guided a-trous filter of SVGF, Schied et al. 2017) — an EXTENSION (DESIGN.md §10
 * f15).  The filter narrows as a pixel converges, so one setting serves 4 samples and 1000.  color, out (may alias color), the
 * guides and rgba are pt_denoise's; moments_dev float[h][w][2] = (m1, m2) as pt_render_moments writes it; length_dev float[h][w]
 * (may be NULL: 1 everywhere), the history length in frames as pt_temporal writes it; out_variance_dev float[h][w] (may be NULL).
 * a' and the hit flag are pt_denoise's (albedo > 1e-3 ? albedo : 1 per channel; a hit when normal != 0);
 * L(c) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b.
 *   Seed, in binary32, one rounding per operation: n = samples_per_frame * len_p;
 *     var_p = n >= 2 ? fmaxf(0, m2 - m1 * m1) / (n - 1) : m2, then fminf(fmaxf(var_p, 0), 1e30f): a NaN counts as 0, the
 *     result is finite (with fewer than two samples a pixel is taken to be as uncertain as it is bright);
 *     i0 = c / a';  v0 = var_p / (L(a') * L(a')): the variance of the mean luminance, carried into demodulated space.
 *   Iteration l = 0 .. iterations-1, step s = 2^l:
 *     g_p = the (1, 2, 1) x (1, 2, 1) mean of v(l) over the 3x3 ADJACENT pixels (whatever s), of which only those inside the
 *       image and with the hit flag of p take part; the mean divides by the weights actually used;
 *     sd_p = sqrt(max(g_p, 0)),  k_p = 1 / (sigma_luminance sd_p + 1e-4);
 *     w_pq = h(dx) h(dy) exp(-|L(i_p) - L(i_q)| k_p - |n_p - n_q|^2 / sigma_normal^2 - |x_p - x_q|^2 / (sigma_position t_p)^2),
 *       the normal and position terms, h, the taps q = p + s (dx, dy) and w = 0 where exactly one of p, q is a miss as in
 *       pt_denoise; the centre tap has weight h(0) h(0); a term with sigma <= 0 is left out;
 *     i(l+1)_p = sum_q w_pq i(l)_q / sum_q w_pq,   v(l+1)_p = sum_q w_pq^2 v(l)_q / (sum_q w_pq)^2.
 *   out = clamp01(i(L) a'), its display word into rgba_dev as pt_denoise packs it; out_variance = v(L) L(a')^2.
 *   iterations = 0: out = color bit for bit, out_variance = var_p.
 * PT_ERR_INVALID: everything pt_denoise refuses (NULL color / guide / out pointer, width or height < 1, iterations outside
 * 0..10, a non-finite sigma); then NULL moments_dev; samples_per_frame not finite or < 1; out_variance_dev equal to an input
 * (color, moments, length or a guide).  No scene needed.  Asynchronous on the context's stream, hence ordered after an earlier
 * pt_render_moments; with PT_OPT_TIMING=1, pt_last_kernel_ms covers all of its launches.  Scratch: pt_denoise's two float[4]
 * frames, the same buffer under the same rule (grown by whichever call needs more, that call synchronises once; a later call of
 * either kind at the same or a smaller size neither allocates nor synchronises).
 * Left out: a spatial variance estimate for short histories (SVGF's 7x7 fallback), per-channel variance, an unclamped output,
 * per-stripe operation in the multi-GPU tile split. */
typedef struct pt_denoise_variance_params {
    int32_t width, height;
    int32_t iterations;                                  /* 0..10                                              */
    float sigma_luminance, sigma_normal, sigma_position; /* <= 0 switches that term off                        */
    float samples_per_frame;                             /* >= 1, finite: samples behind ONE frame of the moments */
    int32_t _pad;
} pt_denoise_variance_params;                            /* 32 bytes                                           */
int pt_denoise_variance(pt_ctx* ctx, const pt_denoise_variance_params* dp, const float* color_dev,
                        const float* moments_dev, const float* length_dev /* may be NULL */,
                        const float* albedo_dev, const float* normal_dev, const float* position_dev,
                        float* out_dev, float* out_variance_dev /* may be NULL */, uint32_t* rgba_dev);

/* ---- temporal reprojection — an EXTENSION ---------------------------------
 * pt_temporal: carries a history of earlier frames into a new frame rendered from a camera that has moved (the first stage of
 * SVGF-style chains), so that a displayed pixel keeps the samples of the frames before it instead of restarting at
 * sample_index = 1.  The scene is static and the camera moves; the hit point pt_render_aux wrote for a pixel is projected into
 * the previous camera, and the history is read there with a bilinear footprint whose taps must lie on the same surface.
 *   colours float[h][w][3] (the accumulator layout), lengths float[h][w] (a history length counts FRAMES, so the host keeps
 *   the samples per frame constant), guides as pt_render_aux writes them (float[4] rows, int32 ids).  prev_* describe the
 *   history as seen from prev_cam; cur_color_dev is the new frame (rendered with sample_index = 1), cur_* its guides.
 * For pixel p = (x, y) of the current frame, with n_p, x_p (xyz) and t_p (.w) its normal and position rows, in binary32 and in
 * this order (vdot(u, v) = fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x)); no other fused multiply-add than the ones written):
 *   1. n_p == (0, 0, 0), a current miss: out = cur, out_length = 1.
 *   2. v = x_p - prev_cam.pos;  a = vdot(v, front), b = vdot(v, right), c = vdot(v, up).  The history is rejected unless a > 0.
 *      fx = fmaf(b / a, sx, (float)w / 2.0f - 0.5f),  fy = fmaf(c / a, sy, (float)h / 2.0f - 0.5f),  with
 *      sx = (float)(w - 1) / (aspect * fov),  sy = (float)(h - 1) / fov  of prev_cam, computed once on the host — the inverse of
 *      the pixel mapping of pt_render's camera ray for an orthonormal basis (every ray passes through pos; an integer fx is a
 *      pixel centre).  The history is rejected when fx or fy is not finite.
 *   3. x0 = floorf(fx), wx = fx - x0 (y likewise); the taps are q = (x0 + i, y0 + j), i, j in 0..1, with the weights
 *      w_q = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy).
 *   4. A tap counts when it is inside the image, w_q > 0, the history pixel is a hit (n_q != 0), the ids are equal (compared
 *      only when both id pointers are given), vdot(n_p, n_q) >= normal_threshold and
 *      fabsf(vdot(n_p, x_q - x_p)) <= plane_tolerance * t_p: its hit point lies within that fraction of the ray distance of the
 *      current pixel's tangent plane.
 *   5. sw = sum of w_q, sc = sum of w_q c_q, sl = sum of w_q len_q over the taps that count (j outer, i inner; fmaf(w, c, sc)).
 *      The history is accepted when sw >= 0.01 (a definition that keeps 1 / sw finite).  Then, with inv = 1.0f / sw:
 *          hist = sc * inv,  n = fminf(sl * inv + 1.0f, max_history),  out = fmaf(cur - hist, 1.0f / n, hist),  out_length = n.
 *      Not accepted (or rejected in 2.): out = cur bit for bit, out_length = 1.
 * prev_color_dev == NULL: there is no history yet; prev_cam and every prev_* are ignored, out = cur bit for bit and
 * out_length = 1 everywhere — a host's first frame goes through the same call as every later one.
 * rgba_dev (may be NULL) receives the 0x00BBGGRR display word of out, as pt_render packs it; there is no clamp, out is a convex
 * combination of its inputs.  out_color_dev may alias cur_color_dev (a lane reads only its own current pixel); the caller
 * ping-pongs the history: out_color_dev == prev_color_dev or out_length_dev == prev_length_dev is refused.
 * PT_ERR_INVALID: NULL ctx, params, cur_* colour / normal / position or out_* pointer; with a history a NULL prev_cam, length,
 * normal or position pointer, exactly one of the two id pointers, or the aliasing above; width or height < 2 (the camera mapping
 * divides by w - 1, h - 1); max_history not finite or < 1; plane_tolerance not finite or < 0; normal_threshold outside -1..1.
 * No scene needed; no scratch, no allocation, no synchronisation.  Asynchronous on the context's stream, hence ordered after
 * the fold of an earlier pt_render (which stays on that stream under PT_OPT_OVERLAP) and after pt_render_aux; the outputs can go
 * straight into pt_denoise.  With PT_OPT_TIMING=1, pt_last_kernel_ms reports its device time.
 * Triangles moved by pt_refit_bvh fail the plane test where they moved and lose their history — except one that slides within its
 * own plane, which passes every test and takes the history of another surface point: pt_temporal_motion (below) is the call for
 * a scene whose triangles move.
 * Out of scope: following specular first hits (a
 * mirror's history is looked up where its surface was, not where its reflection was), per-stripe operation in the multi-GPU
 * tile split (the call is full-frame). */
typedef struct pt_temporal_params {
    int32_t width, height;      /* >= 2 each                                                          */
    float max_history;          /* >= 1: cap on the history length in frames                          */
    float plane_tolerance;      /* >= 0: fraction of t_p a tap's hit point may lie off the tangent plane */
    float normal_threshold;     /* -1..1: smallest dot(n_p, n_q) of a tap on the same surface          */
    int32_t _pad;
} pt_temporal_params;           /* 24 bytes */
int pt_temporal(pt_ctx* ctx, const pt_temporal_params* tp, const pt_camera* prev_cam,
                const float* prev_color_dev, const float* prev_length_dev,
                const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                const float* cur_color_dev,
                const float* cur_normal_dev, const float* cur_position_dev, const int32_t* cur_id_dev,
                float* out_color_dev, float* out_length_dev, uint32_t* rgba_dev);

/* pt_temporal_motion: pt_temporal for a scene whose triangles moved between the two frames (pt_refit_bvh) — an EXTENSION
 * (DESIGN.md §10 f14).  The id pt_render_aux wrote for a pixel names its triangle; the pixel's barycentric coordinates in that
 * triangle NOW, applied to the vertices the triangle had THEN, give where the surface point was, and the history is looked up
 * there.  prev_verts_dev / cur_verts_dev have pt_refit_bvh's layout: float[n_tris][9] = v0, v1, v2 of the triangle whose
 * ORIGINAL id is the row; device memory; rows only 4-byte aligned; the two pointers may be equal.  prev_verts_dev is the scene
 * the prev_* guides were rendered from, cur_verts_dev the scene the cur_* guides were rendered from (for a mesh that was never
 * refit both are its rest pose).  Everything not named here — the buffers, pt_temporal_params, the bilinear footprint, the blend,
 * rgba_dev, the aliasing rules, asynchrony on the context's stream, PT_OPT_TIMING — is pt_temporal's, word for word.
 * For pixel p = (x, y) with normal n_p, position x_p, ray distance t_p and id i_p, in binary32 and in this order
 * (vcross(u, v) = (fmaf(u.y, v.z, -(u.z * v.y)), fmaf(u.z, v.x, -(u.x * v.z)), fmaf(u.x, v.y, -(u.y * v.x))),
 * vmadd(u, s, v) = fmaf(u, s, v) per component, vdot as above; no other fused operation):
 *   1. n_p == (0, 0, 0), a current miss: out = cur, out_length = 1, motion = (0, 0).
 *   2. Where the point was, (x', n'):
 *      static, x' = x_p and n' = n_p, when i_p < 0 (a sphere, or an id that is no triangle), or when the nine words of row i_p
 *        are equal as 32-bit patterns in both vertex buffers: an unmoved surface follows pt_temporal's arithmetic exactly;
 *      i_p >= n_tris: the history is rejected, and neither vertex buffer is read at that row;
 *      moved otherwise, with c0, c1, c2 the current row and p0, p1, p2 the previous one:
 *        e1 = c1 - c0, e2 = c2 - c0, w = x_p - c0;  N = vcross(e1, e2);  nn = vdot(N, N); rejected unless nn > 0 and finite.
 *        inv = 1.0f / nn;  u = vdot(vcross(w, e2), N) * inv;  v = vdot(vcross(e1, w), N) * inv (not clamped); rejected when
 *        either is not finite.
 *        f1 = p1 - p0, f2 = p2 - p0;  x' = vmadd(f2, v, vmadd(f1, u, p0)).
 *        N' = vcross(f1, f2);  nn' = vdot(N', N'); rejected unless nn' > 0 and finite.
 *        k = (vdot(n_p, N) < 0 ? -1.0f : 1.0f) * (1.0f / sqrtf(nn'));  n' = N' * k: the previous triangle's unit normal on the
 *        face the current ray sees.
 *   3. pt_temporal's step 2 on v = x' - prev_cam.pos: a, b, c, fx, fy with the same sx, sy and the same rejections.
 *      motion = (fx - (float)x, fy - (float)y) whenever this step does not reject, whatever the taps then decide; else (0, 0).
 *   4. The footprint and the weights are pt_temporal's.  A tap counts when it is inside the image, w_q > 0, n_q != 0,
 *      prev_id[q] == i_p, vdot(n', n_q) >= normal_threshold and fabsf(vdot(n', x_q - x')) <= plane_tolerance * t_p: the surface
 *      tests run in the previous frame's space, against the previous frame's guides.
 *   5. pt_temporal's step 5.  Not accepted, or rejected above: out = cur bit for bit, out_length = 1.
 * motion_dev (may be NULL): float[h][w][2], where in the previous frame the pixel's surface point was, relative to the pixel.
 * prev_color_dev == NULL: no history yet; as pt_temporal, motion = (0, 0) everywhere, the vertex pointers and n_tris are ignored.
 * PT_ERR_INVALID: everything pt_temporal refuses; with a history also either id pointer NULL (the ids choose the rows), a NULL
 * vertex pointer while n_tris > 0, n_tris >= 2^31, motion_dev equal to any input or output buffer.  n_tris == 0 is valid: every
 * triangle pixel then has no history.  No scene needed; no scratch, no allocation, no synchronisation.
 * Left out: moving spheres (a sphere's pixels are static); history for points that were hidden or off screen in the previous
 * frame (they restart, as under a camera move); the lag of lighting that changes because geometry moved — a shadow that wanders
 * over a static wall keeps its history (max_history is the caller's handle); specular
 * first hits; per-stripe operation in the multi-GPU tile split. */
int pt_temporal_motion(pt_ctx* ctx, const pt_temporal_params* tp, const pt_camera* prev_cam,
                       const float* prev_verts_dev, const float* cur_verts_dev, size_t n_tris,
                       const float* prev_color_dev, const float* prev_length_dev,
                       const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                       const float* cur_color_dev,
                       const float* cur_normal_dev, const float* cur_position_dev, const int32_t* cur_id_dev,
                       float* out_color_dev, float* out_length_dev, uint32_t* rgba_dev,
                       float* motion_dev /* float[h][w][2], may be NULL */);

/* pt_temporal_moments: the luminance moments of pt_render_moments reprojected the way the colour is — an EXTENSION (DESIGN.md
 * §10 f15), what pt_denoise_variance needs beside a history made by pt_temporal / pt_temporal_motion.  The buffers named
 * *_moments_dev are float[h][w][2] = (m1, m2); everything else is the colour call's.  The footprint, the tests of a tap, the
 * acceptance and n = fminf(sl * inv + 1.0f, max_history) are those calls' statements; the payload is (m1, m2) instead of rgb:
 * out = fmaf(cur - hist, 1.0f / n, hist) per component, and out = cur bit for bit where the history is not accepted.  Given the
 * colour buffers (m1, m2, 0) the colour calls write these two values into their first two channels, bit for bit.
 * Both vertex pointers NULL: pt_temporal's rule (ids of both frames or of neither).  Otherwise pt_temporal_motion's rule and
 * requirements (both ids, no NULL vertex pointer while n_tris > 0, n_tris < 2^31).  prev_moments_dev == NULL: no history, out =
 * cur.  No length and no display word is written: the host passes the prev_length_dev of the colour call of the same frame,
 * before it swaps.  out_moments_dev may alias cur_moments_dev; out_moments_dev == prev_moments_dev is refused.  The other errors,
 * asynchrony and PT_OPT_TIMING are pt_temporal's. */
int pt_temporal_moments(pt_ctx* ctx, const pt_temporal_params* tp, const pt_camera* prev_cam,
                        const float* prev_verts_dev, const float* cur_verts_dev, size_t n_tris,
                        const float* prev_moments_dev, const float* prev_length_dev,
                        const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                        const float* cur_moments_dev,
                        const float* cur_normal_dev, const float* cur_position_dev, const int32_t* cur_id_dev,
                        float* out_moments_dev);

/* ---- guide buffers and reprojection for the camera models — an EXTENSION ----------------------------
 * The two calls that carry pt_render_camera's and pt_render_pixels' frames through the image stages: guides under a camera model
 * (for pt_denoise, pt_denoise_variance and the reprojection) and the reprojection into a previous frame of a camera model.  The
 * filters read guides and never a camera, so they serve all five models as they are.
 *
 * pt_render_aux_camera: pt_render_aux under a camera model.  The image is cm's, W x H = cm->width x cm->height (as
 * pt_render_camera reads pt_params); of params only cull_backfaces and tri_col are read.  The four outputs have pt_render_aux's
 * layouts and meanings, a miss is all zero with id -1.
 *   The ray of pixel pix = y * W + x is, bit for bit, the row pt_camera_rays writes for pix under PT_CAMF_CENTRE with lens_radius
 *   taken as 0: no jitter, no lens draw, no random number read.  For PT_CAM_THIN_LENS that is the ray through the lens centre — the
 *   surface that is sharp in the rendered frame.  cm->flags is checked for unknown bits and otherwise ignored, cm->lens_radius is
 *   range-checked and otherwise ignored.  With PT_CAM_PINHOLE the four buffers are pt_render_aux's bit for bit.
 *   The hit is pt_render_aux's: the binary closest-hit walk, then the spheres, the material row or tri_col.  A pixel without a ray
 *   (d == (0, 0, 0): outside the fisheye's image circle) is not walked and writes a miss.
 * Errors, in this order, nothing written on any of them: NULL ctx PT_ERR_INVALID; a NULL cam, cm, params or float buffer
 * PT_ERR_INVALID; pt_camera_rays' checks of cm for the whole image (n = W * H, first_pixel 0) in its order and wording, prefixed
 * pt_render_aux_camera:; no BVH PT_ERR_NO_SCENE; Woop records PT_ERR_UNSUPPORTED.  Asynchronous on the context's stream, ordered
 * after pt_refit_bvh; no scratch, no allocation, no synchronisation; with PT_OPT_TIMING=1, pt_last_kernel_ms covers it. */
int pt_render_aux_camera(pt_ctx* ctx, const pt_camera* cam, const pt_camera_model* cm, const pt_params* params,
                         float* albedo_dev, float* normal_dev, float* position_dev, int32_t* id_dev /* may be NULL */);

/* pt_temporal_camera: pt_temporal / pt_temporal_motion with the history seen through a camera MODEL: prev_cam and prev_cm are the
 * camera and the model the prev_* guides and colours were rendered under (pt_render_aux_camera, pt_render_camera).  The current
 * camera is not an argument: the current guides hold world positions.  Everything not named here — the buffers,
 * pt_temporal_params, steps 1 and 3 to 5, the blend, rgba_dev, the aliasing rules, prev_color_dev == NULL, asynchrony,
 * PT_OPT_TIMING — is pt_temporal's or pt_temporal_motion's, word for word.
 * Where the point was, (x', n').  With a non-NULL vertex pointer: pt_temporal_motion's step 2 and its requirements (both id
 * pointers, no NULL vertex pointer while n_tris > 0, n_tris < 2^31).  With both vertex pointers NULL: x' = x_p and n' = n_p for
 * every pixel, no row is read, n_tris is ignored, and the ids are given for both frames or for neither (pt_temporal's rule).
 * motion_dev (may be NULL, in either mode): (fx - x, fy - y), or (0, 0) where the projection rejects, as pt_temporal_motion
 * defines it; it may not be one of the other buffers.
 * The projection replaces step 2 of pt_temporal and is chosen by prev_cm->model.  v = x' - prev_cam.pos; a = vdot(v, front),
 * b = vdot(v, right), c = vdot(v, up); cx = (float)W / 2.0f - 0.5f, cy = (float)H / 2.0f - 0.5f.  binary32 throughout, the only
 * fused operations are the ones written; constants marked "host" are computed once on the host in binary32, one rounding per
 * operation.
 *   PT_CAM_PINHOLE, PT_CAM_THIN_LENS   pt_temporal's step 2, unchanged: both models' guide rays pass through pos along dir0.  With
 *                     these two the call is pt_temporal (no rows, no motion_dev) or pt_temporal_motion (rows) bit for bit.
 *   PT_CAM_ORTHO      rejected unless a > 0.  kx = (float)W / (ortho_height * aspect), ky = (float)H / ortho_height (host);
 *                     fx = fmaf(b, kx, cx), fy = fmaf(c, ky, cy).
 *   PT_CAM_FISHEYE    s = sqrtf(fmaf(c, c, b * b)); rejected when a == 0 and s == 0.  theta = atan2f(s, a), half = fisheye_fov /
 *                     2.0f (host); rejected when theta > half.  kf = ((float)min(W, H) / 2.0f) / half (host); rho = theta * kf;
 *                     k = s > 0 ? rho / s : 0; fx = fmaf(b, k, cx), fy = fmaf(c, k, cy).  There is no a > 0 test: a fisheye
 *                     wider than 180 degrees sees behind itself.
 *   PT_CAM_EQUIRECT   h = sqrtf(fmaf(b, b, a * a)); rejected when h == 0 and c == 0.  lon = atan2f(b, a), lat = atan2f(c, h);
 *                     fx = fmaf(lon, (float)W / 6.28318548f, (float)W / 2.0f), fy = fmaf(lat, (float)H / 3.14159274f,
 *                     (float)H / 2.0f), both factors host: the inverse of pt_camera_rays' model, an integer coordinate is a
 *                     texel centre.
 * In every model the history is rejected when fx or fy is not finite (atan2f is the device library's: the coordinates of the
 * three models with an angle are not pinned bit for bit, tests/test_gpu_camera_guides.py holds them to 1e-3 pixel).
 * PT_ERR_INVALID: everything pt_temporal refuses, in its order; then, with a history and right behind the NULL prev_* pointers:
 * a NULL prev_cm; pt_camera_rays' checks of prev_cm for the whole image, prefixed pt_temporal_camera:; prev_cm->width or height
 * other than the parameters'; then the ids, the aliasing, and with rows pt_temporal_motion's checks; motion_dev equal to another
 * buffer.  Without a history prev_cam and prev_cm are ignored.
 * Left out: horizontal wrap of the equirectangular taps at the +-180 degree seam (a footprint that straddles it uses its
 * in-image taps); a moments variant (a host passes the moments as the first two channels of a three-channel buffer, see
 * pt_temporal_moments); `pt_app --camera` with --denoise-out, --temporal-out or the motion options (still refused). */
int pt_temporal_camera(pt_ctx* ctx, const pt_temporal_params* tp, const pt_camera* prev_cam, const pt_camera_model* prev_cm,
                       const float* prev_verts_dev, const float* cur_verts_dev, size_t n_tris,
                       const float* prev_color_dev, const float* prev_length_dev,
                       const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                       const float* cur_color_dev,
                       const float* cur_normal_dev, const float* cur_position_dev, const int32_t* cur_id_dev,
                       float* out_color_dev, float* out_length_dev, uint32_t* rgba_dev,
                       float* motion_dev /* float[h][w][2], may be NULL */);

/* ---- display: exposure metering and tone mapping, an EXTENSION ---------------------------------
 * The last stage of a frame: any float[H][W][3] buffer (an accumulator, PT_RAYS_HDR or clamped; a denoiser's or the temporal
 * filter's output) becomes display words on the device, under an exposure a meter found on the device.  render, (temporal),
 * (denoise), pt_meter, pt_tonemap then run on one stream with no host round trip.  Everything is binary32 / integer arithmetic
 * with plain *, + and the correctly rounded / (no fused operation), so numpy restates it bit for bit (tests/tonemap_ref.py).
 *
 * pt_tonemap, per pixel and channel c of color_dev:
 *   exposure  e = tp->exposure; with exposure_dev, e = tp->exposure * exposure_dev[0], read on the device; a product that is not
 *             finite or is <= 0 falls back to e = tp->exposure
 *   input     x = c * e, then x = x > 0 ? fminf(x, 65536.0f) : 0      (a NaN and a negative become 0, +inf becomes 65536)
 *   curve     PT_TONE_CLAMP     y = fminf(x, 1)
 *             PT_TONE_REINHARD  on the luminance, so the hue is kept:  L = (0.2126f x.r + 0.7152f x.g) + 0.0722f x.b,
 *                               s = (1.0f + L * iw2) / (1.0f + L),  y = fminf(x * s, 1),  where iw2 = 0 for white == +inf (plain
 *                               Reinhard) and 1.0f / (white * white) otherwise, computed on the host in binary32
 *             PT_TONE_ACES      the Narkowicz fit, per channel:  a = x * (2.51f * x + 0.03f),  b = x * (2.43f * x + 0.59f) + 0.14f,
 *                               y = fminf(a / b, 1)
 *   out_dev   float[H][W][3] receives y, the curve's output BEFORE the transfer (for hosts with an encoding of their own)
 *   rgba_dev  uint32[H][W] receives 0x00BBGGRR of three codes.  PT_XFER_LINEAR: the truncating pack of pt_render's display words,
 *             (unsigned char)(255.0f * y) — so CLAMP + LINEAR + exposure 1 over an accumulator gives the words pt_render writes
 *             under PT_FLAG_WRITE_RGBA.  PT_XFER_SRGB / PT_XFER_GAMMA22: code = the number of k in 1..255 with y >= T[k], T the
 *             table of pt_tonemap_thresholds: round-to-nearest of the encoded value with no pow on the device.
 * out_dev may alias color_dev (a thread reads its pixels before it writes them); at least one of out_dev, rgba_dev is given.
 * One launch.  Where W * H is a multiple of 4 and every buffer given is 16-byte aligned a thread takes four pixels as three 16-byte
 * loads and writes one 16-byte store of four words; otherwise one pixel per thread.  Both routes give the same bits.  The tables
 * (2 KB) are uploaded to the context by the first call that needs them; no allocation afterwards.
 * Errors, in this order, PT_ERR_INVALID each: NULL ctx; a NULL tp or color_dev, or out_dev and rgba_dev both NULL; width or height
 * < 1, or W * H >= 2^32; a curve or a transfer that is not one of the three; an exposure that is not finite or is <= 0; under
 * PT_TONE_REINHARD a white that is not > 0 (a NaN included; +inf is plain Reinhard).  Nothing is written by a refused call.
 *
 * pt_tonemap_thresholds: T[0] = 0 and T[k] = eotf((k - 0.5) / 255) for k = 1..255, evaluated in double and rounded once to binary32;
 * PT_XFER_SRGB: eotf(v) = v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4);  PT_XFER_GAMMA22: pow(v, 2.2).  Strictly
 * increasing.  Host only, no context.  PT_ERR_INVALID for a NULL out256 or another transfer (PT_XFER_LINEAR has no table).
 *
 * pt_meter leaves the exposure for a frame in state_dev, float[4] on the device, without the host seeing it:
 *   state[0] the exposure in use   [1] this frame's target   [2] the metered luminance Lavg   [3] (float) the pixels that took part
 *   histogram 256 bins of L = (0.2126f r + 0.7152f g) + 0.0722f b of the unscaled colour over 2^-16 .. 2^16, eight per octave, from
 *             the float's own bits (a piecewise-linear logarithm: integer arithmetic).  A pixel whose L is not finite or is < 2^-16
 *             is not metered; L >= 65536 goes to bin 255; otherwise bin = (float_as_uint of L >> 20) - ((127 - 16) << 3).
 *   trim      n = the pixels metered; lo = (uint64)((double)low_pct * (double)n), hi likewise from high_pct; hi <= lo: lo = 0,
 *             hi = n.  With inclusive prefix counts cum, bin b takes part with w_b = max(0, min(cum_b, hi) - max(cum_(b-1), lo)).
 *   average   S = sum w_b (2b + 1), Wt = sum w_b in 64-bit integers; p = (double)S / (double)(16 Wt) - 16.0, i = floor of p,
 *             Lavg = (float)ldexp(1.0 + (p - i), i): the inverse of the same logarithm, with no exp2 or log2
 *   target    fminf(fmaxf(key / Lavg, min_exposure), max_exposure).  Wt == 0: Lavg = 0 and the target is the previous state[0] if
 *             that is finite and > 0 (also under reset: zero the state before a first frame that may be black), else 1, clamped alike.
 *   in use    state[0] = (reset or the previous state[0] is not finite or is <= 0) ? target : prev + (target - prev) * adapt
 *   A uniform 0.18 grey meters as bin 107, Lavg = 0.1796875.
 * Two launches: a histogram pass over min(ceil(W H / 256), 256) blocks of 256 threads, each thread striding over pixels (four at a
 * time as three 16-byte loads where W * H is a multiple of 4 and color_dev is 16-byte aligned), counting into a 257-entry LDS
 * histogram by integer LDS adds — the 257th entry counts the unmetered pixels — and storing the block's histogram into the context's
 * scratch [blocks][257] with plain stores (no global atomics; integer adds give the same counts in any order); then one 256-thread
 * block that adds the partial histograms per bin, scans them and writes the four floats from one thread.  No copy back, no
 * synchronisation, no allocation after the first call: the scratch is 256 x 257 x 4 bytes (263 KB), freed by pt_destroy.
 * Errors, in this order, PT_ERR_INVALID each: NULL ctx; a NULL mp, color_dev or state_dev; width or height < 1, or W * H >= 2^32; a
 * key that is not finite or is <= 0; percentages outside 0 <= low_pct < high_pct <= 1; exposure limits that are not finite with
 * 0 < min_exposure <= max_exposure; an adapt outside 0..1.  Nothing is written by a refused call, the state included.
 *
 * Both calls are asynchronous on the context's stream — pt_tonemap after pt_meter reads the state the meter wrote — need no scene,
 * and with PT_OPT_TIMING=1 pt_last_kernel_ms covers each of them.
 * Left out: dithering, bloom, per-channel or local operators, a log-domain adaptation rate, display words fused into the folds of
 * the render calls, a display-space error criterion for pt_select_pixels. */
enum { PT_TONE_CLAMP = 0, PT_TONE_REINHARD = 1, PT_TONE_ACES = 2 };
enum { PT_XFER_LINEAR = 0, PT_XFER_SRGB = 1, PT_XFER_GAMMA22 = 2 };
typedef struct pt_tonemap_params {
    int32_t width, height;   /* >= 1, W * H < 2^32 */
    int32_t curve;           /* PT_TONE_* */
    int32_t transfer;        /* PT_XFER_* */
    float exposure;          /* finite, > 0: scale on linear radiance */
    float white;             /* PT_TONE_REINHARD: the scaled luminance shown as white; > 0, +inf = plain Reinhard; ignored otherwise */
} pt_tonemap_params;         /* 24 bytes */
int pt_tonemap(pt_ctx* ctx, const pt_tonemap_params* tp, const float* color_dev,
               const float* exposure_dev /* may be NULL: float[1], e.g. pt_meter's state */,
               float* out_dev /* may be NULL; may alias color_dev */, uint32_t* rgba_dev /* may be NULL; not both */);
typedef struct pt_meter_params {
    int32_t width, height;
    float key;                        /* finite, > 0: the luminance the metered average is shown at (0.18) */
    float low_pct, high_pct;          /* 0 <= low < high <= 1: share of the metered pixels ignored below / kept up to */
    float min_exposure, max_exposure; /* finite, 0 < min <= max */
    float adapt;                      /* 0..1: weight of this frame's target in the exposure in use; 1 = jump */
} pt_meter_params;                    /* 32 bytes */
int pt_meter(pt_ctx* ctx, const pt_meter_params* mp, const float* color_dev, float* state_dev /* float[4], device */, int reset);
int pt_tonemap_thresholds(int transfer, float* out256);

/* ---- measurement --------------------------------------------------------------- */
int pt_get_counters(pt_ctx* ctx, pt_counters* out);
/* Schedule statistics of the last instrumented launch of the persistent wide walk
 * (PT_OPT_COUNTERS=1), summed over waves; up to PT_WAVE_STATS values:
 * [0] node-step iterations  [1] lanes active in them  [2] record-step iterations  [3] lanes
 * [4] shading passes        [5] lanes                 [6] path-start passes       [7] lanes
 * [8] outer-loop iterations  [9] traversal-stack pushes that overflowed the LDS window into
 * private memory (PT_OPT_LDS_STACK).  A wave-iteration with all 64 lanes active is 100 % use.
 * PT_KERNEL_WAVEFRONT: [0]-[3] and [6]-[9] are the extend stage's ([6]/[7] = refill passes), its
 * shade stage runs one lane per live path ([5] = the rays of the any-hit launch, PT_OPT_LAST_ANYHIT 2, else 0); [4] counts the 64-ray groups the bounce-0
 * packet walk (PT_OPT_FIRST_WALK 1) walked — 0 when bounce 0 ran the per-lane walk — and that
 * launch books its wave node / record steps and the lanes of their masks in [0]-[3].
 * [10] PT_KERNEL_WAVEFRONT with PT_OPT_ROOT_CULL 2: the rays the shade stage kept out of the extend queue (they
 * are part of pt_counters.rays, not of [5]); 0 everywhere else.
 * [11] PT_KERNEL_WAVEFRONT with PT_OPT_LAST_OCCLUDERS 2: the last-segment rays one of the tree's occluders decided in the shade stage
 * (part of pt_counters.rays, not of [5] or [10]); 0 everywhere else. */
#define PT_WAVE_STATS 12
int pt_get_wave_stats(pt_ctx* ctx, uint64_t* out, int n);
int pt_last_kernel_ms(pt_ctx* ctx, float* ms_out);   /* needs PT_OPT_TIMING=1 */
/* Device time of the last timed pt_render (PT_OPT_TIMING=1) by stage, from HIP events recorded on the
 * context's stream between the launches: out[PT_STAGE_x] = milliseconds spent in that kind of launch,
 * summed over the call (PT_KERNEL_WAVEFRONT runs `depth` extend and `depth` shade launches).  The
 * reference's only timer is uf::GpuTimer around the whole launch (utilfun.hpp:44-79). */
enum {
    PT_STAGE_NONE = 0,      /* (start marker)                                                   */
    PT_STAGE_FRAME = 1,     /* the frame kernel of PT_KERNEL_MEGA_BVH2 / PT_KERNEL_PERSISTENT      */
    PT_STAGE_GENERATE = 2,  /* wavefront: prepare + camera rays                                   */
    PT_STAGE_EXTEND = 3,    /* wavefront: closest-hit walks, all bounces                          */
    PT_STAGE_SHADE = 4,     /* wavefront: spheres + shading + compaction, all bounces             */
    PT_STAGE_FOLD = 5,      /* k_fold_samples: sample colours -> running mean + display word      */
    PT_STAGE_COUNT = 6
};
int pt_get_stage_ms(pt_ctx* ctx, float* out, int n);
/* PT_KERNEL_AUTO's pick for the configuration of the last pt_render: *kernel = PT_KERNEL_PERSISTENT or
 * PT_KERNEL_WAVEFRONT once decided (PT_KERNEL_AUTO while the two trials are still running), and the two trial times. */
int pt_auto_choice(pt_ctx* ctx, int* kernel, float* ms_persistent, float* ms_wavefront);
/* Surface-area cost of the 4-wide tree on the context (measurement; what a random ray is expected to fetch):
 * *node_visits = (area of the root + of every child box that leads to a wide node) / area of the root,
 * *tri_tests   = sum over leaves of (area of the leaf's box x its triangle records) / area of the root.
 * Areas are those of the quantised boxes the walk tests.  Synchronises the context's stream. */
int pt_tree_cost(pt_ctx* ctx, double* node_visits, double* tri_tests);
/* The item buffer of the tree on the context, read-only (measurement; what tests/tree_audit.py reads): *items_dev = its device
 * pointer, 64-byte items laid out [binary nodes][records][wide nodes] with *n_binary, *n_records and *n_wide items in the three
 * sections (any of the counts may be NULL), *wide_depth = levels of the 4-wide tree.  The words of every item are written down in
 * DESIGN.md 3.5.  *n_binary is the size of the section (what the links are relative to): a device-built tree with
 * PT_OPT_LEAF_MAX > 1 keeps the binary nodes below its multi-record leaves there, unreachable.  Synchronises the context's stream,
 * so a pending pt_refit_bvh is complete; the pointer is valid until the tree is replaced (pt_upload_bvh, pt_build_bvh) or the
 * context destroyed.  PT_ERR_NO_SCENE without a tree, PT_ERR_INVALID for a NULL ctx or items_dev. */
int pt_tree_items(pt_ctx* ctx, const void** items_dev, uint64_t* n_binary, uint64_t* n_records,
                  uint64_t* n_wide, uint32_t* wide_depth);
int pt_scene_info(pt_ctx* ctx, uint64_t* n_inner, uint64_t* n_tri_refs,
                  uint64_t* n_leaves, uint32_t* max_depth, uint64_t* device_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
