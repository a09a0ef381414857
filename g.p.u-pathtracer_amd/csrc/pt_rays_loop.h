// pt_rays_loop.h — the path loop over (sample, row) slots that pt_render_rays and pt_render_camera share, written once: the kernel
// template k_rays_loop<V, START>, whose instantiations over the two path starts are k_render_rays<V> (pt_k_rays.hip, START = KRays)
// and k_render_camera<V> (pt_k_camera.hip, START = KCamRays).  DESIGN.md §10 f10, f17.  The loop is the kernel itself and not a
// __device__ function two kernels call: behind a call boundary hipcc schedules all 19 k_render_rays differently (same registers,
// other instruction streams), and those kernels are pinned instruction for instruction (profiles/r25_render_camera.txt).
//
// The loop is k_trace_persist_bvh2 (pt_k_persist.hip) with another path start: persistent waves draw chunks of (sample, row)
// slots from the context's sharded queue, idle lanes take the next slots by a ballot + prefix count, lanes with a segment in flight
// run the resumable walk, lanes whose walk finished shade.  A slot q is sample q / n of row q % n.  Where its path starts is the
// START's business (R.start: the first segment and the random stream, left behind the camera's two jitter draws): KRays reads a
// caller's ray, KCamRays (pt_k_camera.hip) makes a camera model's in registers.  From there on it is path_shade and the walks of the
// frame kernels.  What the frame kernels do not have and this loop does: a guard in front of the walk (a ray that is not finite or has
// no direction ends as a first-segment miss) and, in the NEE instantiations, the shadow ray of PT_FLAG_NEE as a second walk of the
// same lane — the loop of pt_get_sample (pt_kernels.h) laid out over the phases, which the frame kernel leaves to the other two
// families.  A start travels as the second kernel argument: KParams stays the first one, at offset 0, for PT_KARGS and
// pt_closest_sphere, and keeps its layout.  It has n (rows), out (float[n][3]: the running means), hdr (PT_RAYS_HDR).
#pragma once
#include "pt_kernels.h"

struct KRays {
    const float4* __restrict__ rays;   // [n][2]: (o.xyz, ignored) (d.xyz, ignored)
    float* __restrict__ out;           // [n][3] running mean of the samples' radiance
    unsigned long long first_index;    // RNG key of ray 0
    uint32_t n;
    int hdr;                           // PT_RAYS_HDR: the fold does not clamp

    // the ray as it stands in the buffer, with the RNG of pixel first_index + ray
    template <class PS>
    __device__ __forceinline__ void start(const KParams& P, uint32_t s_idx, uint32_t ray, PS& ps) const {
        const float4 a = pt_sld4(rays + 2 * (size_t)ray), b = pt_sld4(rays + 2 * (size_t)ray + 1);
        ps.o = V3(a.x, a.y, a.z);
        ps.d = V3(b.x, b.y, b.z);
        // the stream a camera path of this (frame, pixel) sees behind its two jitter draws (path_begin_hashed)
        ps.rng = pt_rng_init(pt_wang64(P.frame + s_idx), first_index + ray);
        ps.rng.n = 2;
    }
};

enum { RP_IDLE = 0, RP_TRAV = 1, RP_SHADE = 2, RP_MISS = 3 };   // RP_MISS: shaded as a first segment that hit nothing, never walked

// pt_accumulate, or with HDR the same running mean without its clamp: a = (a * (N - 1) + col) * (1 / N), N == 1 overwrites
template <bool HDR>
__device__ __forceinline__ void rays_accumulate(float& ax, float& ay, float& az, v3 col, uint64_t N) {
    if (!HDR) { pt_accumulate(ax, ay, az, col, N); return; }
    const float fm1 = (float)(N - 1), inv = 1.0f / (float)N;
    if (N == 1) { ax = 0.f; ay = 0.f; az = 0.f; } else { ax *= fm1; ay *= fm1; az *= fm1; }
    ax = (ax + col.x) * inv;
    ay = (ay + col.y) * inv;
    az = (az + col.z) * inv;
}

__device__ __forceinline__ bool rays_finite(v3 a) {
    return fabsf(a.x) <= PT_F32_MAX && fabsf(a.y) <= PT_F32_MAX && fabsf(a.z) <= PT_F32_MAX;   // false for a NaN
}

// NEE: the lane can walk the shadow ray path_shade asks for (PT_FLAG_NEE) before it goes on with the path
// MIS: ... and path_shade weighs that ray against the bounce ray (PT_FLAG_MIS); only with NEE
// V: the word of pt_variants.h (PV_*; rays_exists: what is instantiated)
template <uint32_t V, class START>
__global__ void __launch_bounds__(PT_BLOCK, pv_occ(V)) k_rays_loop(const KParams P, const START R) {
    constexpr bool NEE = pv_nee(V), MIS = pv_mis(V);
    constexpr int LSTK = pv_lstk(V), ALG = pv_alg(V), ENV = pv_env(V);
    // sphere attributes + centres for the shading code (see path_shade): the table of k_trace_persist_bvh2, filled from the device
    // array (the first PT_KSPHERES spheres there are the ones in the kernel arguments; rows past n_spheres are never read)
    if (P.sph_tab >= 0 && (int)threadIdx.x < 11 * min(P.sc.n_spheres, PT_KSPHERES)) {
        const float v = ((const float*)P.sc.spheres)[threadIdx.x];
        ((float*)s_dyn)[P.sph_tab + threadIdx.x] = v;
        if (threadIdx.x % 11 < 4) ((float*)s_dyn)[P.sph_tab + 88 + 4 * (threadIdx.x / 11) + threadIdx.x % 11] = v;
    }
    __syncthreads();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    TravOverflow<LSTK> stk_ovf;
    TravStack<LSTK, PT_BLOCK> stk(__builtin_amdgcn_readfirstlane(tid & ~63), stk_ovf);
    const bool cull = P.cull != 0;
    const unsigned long long total = (unsigned long long)R.n * (P.samples ? P.spp : 1u);   // (the launcher keeps it below 2^32)

    uint32_t chunk_next = 0, chunk_end = 0;  // wave-uniform
    bool queue_empty = false;                // wave-uniform
    int shard = (int)(blockIdx.x & (PT_SHARDS - 1));
    const uint32_t chunk = (uint32_t)P.chunk;
    const uint32_t shard_chunks = (uint32_t)(((total + chunk - 1) / chunk + PT_SHARDS - 1) / PT_SHARDS);

    int phase = RP_IDLE;
    uint32_t ray = 0, s_idx = 0;
    PathStateOf<MIS> ps;
    TravState ts;
    ps.o = ps.d = ps.mask = ps.accu = V3(0.f, 0.f, 0.f);
    ps.depth = 0; ps.rng.s0 = ps.rng.s1 = ps.rng.n = 0; ps.nee_mask = 0;
    if constexpr (MIS) ps.pb = 0.f;
    ts.idx = ts.idy = ts.idz = ts.oodx = ts.oody = ts.oodz = 0.f;
    ts.node = PT_SENTINEL; ts.leaf = 0; ts.sp = 0;
    ts.h = pt_no_hit();
    // NEE: the shadow ray in flight (sh & 1) instead of the path's own segment, which waits in ps; sh & 2: the path ended with the
    // bounce that asked for it
    int sh = 0;
    v3 sh_o = V3(0.f, 0.f, 0.f), sh_d = sh_o, sh_con = sh_o;
    float sh_tmax = 0.f;
    TravCount tc;

    for (;;) {
        // ---- A. refill idle lanes (all 64 lanes are converged here)
        const unsigned long long idle = __ballot(phase == RP_IDLE);
        const int n_idle = __popcll(idle);
        const int n_busy = __popcll(__ballot(phase == RP_TRAV));
        if (!queue_empty && (n_idle >= P.refill || (n_idle > 0 && n_busy == 0))) {
            if (chunk_next == chunk_end) {
                // shard s owns chunks s, s + 8, ...; an empty shard is left for the next one (k_trace_persist_bvh2)
                for (int tries = 0; tries < PT_SHARDS; tries++) {
                    uint32_t k = 0;
                    if (lane == 0) k = atomicAdd(P.queue + shard * PT_SHARD_STRIDE, 1u);
                    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
                    const unsigned long long first = ((unsigned long long)k * PT_SHARDS + (unsigned long long)shard) * chunk;
                    if (k < shard_chunks && first < total) {
                        chunk_next = (uint32_t)first;
                        chunk_end = (uint32_t)min(first + chunk, total);
                        break;
                    }
                    shard = (shard + 1) & (PT_SHARDS - 1);
                }
                if (chunk_next == chunk_end) queue_empty = true;
            }
            const uint32_t avail = chunk_end - chunk_next;
            const uint32_t take = min((uint32_t)n_idle, avail);
            if (phase == RP_IDLE) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (rank < take) {
                    const uint32_t q = chunk_next + rank;   // < total
                    s_idx = q / R.n;
                    ray = q - s_idx * R.n;
                    R.start(P, s_idx, ray, ps);
                    ps.mask = V3(1.f, 1.f, 1.f);
                    ps.accu = V3(0.f, 0.f, 0.f);
                    ps.depth = 0;
                    ps.nee_mask = 0;
                    sh = 0;
                    ts.h = pt_no_hit();
                    // the guard: only a finite ray with a direction is ever walked or tested against a sphere
                    const bool good = rays_finite(ps.o) && rays_finite(ps.d) && !(ps.d.x == 0.f && ps.d.y == 0.f && ps.d.z == 0.f);
                    if (P.depth == 0) {
                        phase = RP_SHADE;
                    } else if (!good) {
                        phase = RP_MISS;
                    } else if (P.sc.has_bvh) {
                        trav_begin(ts, ps.o, ps.d, stk, ALG >= 2 ? P.sc.wide_root : 0);
                        phase = RP_TRAV;
                    } else {
                        phase = RP_SHADE;
                    }
                }
            }
            chunk_next += take;
        }

        // ---- B. closest-hit walk for the lanes with a segment (or a shadow ray) in flight
        {
            const int n_dead = queue_empty ? __popcll(__ballot(phase == RP_IDLE)) : 0;
            if (phase == RP_TRAV) {
                const v3 wo = NEE && (sh & 1) ? sh_o : ps.o, wd = NEE && (sh & 1) ? sh_d : ps.d;
                const bool fin = (ALG >= 2) ? trav_run_wide<TW_DYN | (ALG == ALG_WIDE_WOOP ? TW_WOOP : 0u)>(ts, P.sc, wo, wd, cull, stk, tc, n_dead, P.batch)
                                            : trav_run_unified<TW_DYN>(ts, P.sc, wo, wd, cull, stk, tc, n_dead, P.batch);
                if (fin) phase = RP_SHADE;
            }
        }

        // ---- C. shade finished segments
        if (phase >= RP_SHADE) {
            v3 col = V3(0.f, 0.f, 0.f);
            bool done, walk_shadow = false;
            if (P.depth == 0) {
                done = true;
            } else if (phase == RP_MISS) {
                // path_shade_hit's miss branch for the first segment: the background, by the rule of the flags.  bk_color even with an
                // environment map on the context (pt_upload_environment): such a ray has no direction to look up (include/ptmi.h)
                col = V3(P.bk[0], P.bk[1], P.bk[2]);
                if (P.flags & PT_FLAG_MISS_KEEPS_PATH) col = vadd(ps.accu, vmul(ps.mask, col));
                done = true;
            } else if (NEE && (sh & 1)) {
                // the shadow ray's walk is back (pt_get_sample): unoccluded up to the light -> its contribution joins the gathered light
                if (!(ts.h.t < sh_tmax)) ps.accu = vadd(ps.accu, sh_con);
                done = (sh & 2) != 0;
                col = ps.accu;   // (a path that ended with that bounce returned the gathered light: path_shade_hit's last line)
                sh = 0;
            } else {
                NeeReq req;
                req.want = false;
                done = path_shade<ENV, MIS>(P, ps, ts.h, col, P.sph_tab, NEE && (P.flags & PT_FLAG_NEE) ? &req : nullptr);
                if (NEE && req.want) {
                    if (P.sc.has_bvh) {
                        walk_shadow = true;
                        sh = done ? 3 : 1;
                        sh_o = req.o; sh_d = req.d; sh_con = req.contrib; sh_tmax = req.t_max;
                    } else {   // no triangle can be in the way
                        ps.accu = vadd(ps.accu, req.contrib);
                        if (done) col = ps.accu;
                    }
                }
            }
            if (NEE && walk_shadow) {
                trav_begin(ts, sh_o, sh_d, stk, ALG >= 2 ? P.sc.wide_root : 0);
                phase = RP_TRAV;
            } else if (!done) {
                if (P.sc.has_bvh) {
                    trav_begin(ts, ps.o, ps.d, stk, ALG >= 2 ? P.sc.wide_root : 0);
                    phase = RP_TRAV;
                }  // else: stays RP_SHADE with the (miss) hit record, shaded again next round
            } else if (P.samples) {
                pt_sst3(pt_sample_ptr(P, s_idx, (size_t)ray), col);   // read once, by the fold
                phase = RP_IDLE;
            } else {
                // one sample per launch: folded straight into the caller's running mean
                float* acc = R.out + 3 * (size_t)ray;
                float ax = 0.f, ay = 0.f, az = 0.f;
                if (P.sample_index != 1) { ax = acc[0]; ay = acc[1]; az = acc[2]; }
                if (R.hdr) rays_accumulate<true>(ax, ay, az, col, P.sample_index);
                else rays_accumulate<false>(ax, ay, az, col, P.sample_index);
                acc[0] = ax; acc[1] = ay; acc[2] = az;
                phase = RP_IDLE;
            }
        }

        if (queue_empty && !__ballot(phase != RP_IDLE)) break;
    }
}
