// pt_variants_check.cpp — every request has a kernel and every kernel a request: a CPU program with its own main, no HIP library
// (`make variants_check`, SAN=1 for the address and undefined-behaviour sanitizers; tests/test_variants.py runs both).
// It loops over everything plan_call, wave_plan and pt_render_rays (ptmi.hip, pt_k_wave.hip) can hand the request functions of
// pt_variants.h, asserts that each resulting word satisfies its family's _exists — with_variant (pt_ctx.h) would answer
// hipErrorInvalidValue for any other — and, the other way round, that every word that exists came out of some request.
#include <cstdio>
#include <set>
#include <vector>

#include "pt_variants.h"

static int n_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (n_failed++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                       \
    } while (0)

struct Family {
    const char* name;
    bool (*exists)(uint32_t);
    int n_bits;
    long requests = 0;
    std::vector<char> seen = std::vector<char>(1u << n_bits, 0);   // by word
    void request(uint32_t v) {
        requests++;
        if (v >= seen.size() || !exists(v)) {
            if (n_failed++ < 20) std::printf("FAILED %s: a request asks for word 0x%x, which is not instantiated\n", name, v);
        } else seen[v] = 1;
    }
    void report() const {
        int words = 0;
        for (uint32_t v = 0; v < seen.size(); v++) {
            words += seen[v];
            if (exists(v) && !seen[v] && n_failed++ < 20) std::printf("FAILED %s: no request runs the instantiated word 0x%x\n", name, v);
        }
        std::printf("%-26s %9ld requests, %3d distinct words, %3d kernels\n", name, requests, words, variant_count(exists, n_bits));
    }
};

int main() {
    Family mega{"k_trace_mega_bvh2", mega_exists, PV_BITS}, persist{"k_trace_persist_bvh2", persist_exists, PV_BITS},
        rays{"k_render_rays", rays_exists, PV_BITS}, query{"k_query_rays", query_exists, QV_BITS}, extend{"k_wf_extend", extend_exists, WX_BITS},
        shade{"k_wf_shade", shade_exists, WS_BITS}, last_any{"k_wf_shade_last_any", shade_last_any_exists, WS_BITS},
        fused{"k_wf_extend_packet_shade", fused_exists, WS_BITS};
    const int occs[] = {4, 5, 6, 8}, lstks[] = {16, 24, 72};   // PT_OPT_OCCUPANCY; PT_OPT_LDS_STACK (0 = all 72 entries)
    const int kernels[] = {PT_KERNEL_MEGA_BVH2, PT_KERNEL_PERSISTENT, PT_KERNEL_WAVEFRONT};   // the option, or PT_KERNEL_AUTO's pick

    // pt_render (plan_call): the walk is choose_walk's (0 .. 4; 3 = Woop records), the map env_code's.  The pipeline is possible
    // (wave_ok) only with walk 2 and without a map; PT_FLAG_MIS comes with PT_FLAG_NEE, is refused over Woop records and runs the megakernel.
    std::set<int> wave_calls;   // (count, nee, deep stack, moments) of the calls that run the pipeline
    for (int kernel : kernels)
        for (int walk = ALG_WHILE; walk <= ALG_WIDE_PEND; walk++)
            for (int map = ENV_NONE; map <= ENV_LIGHT; map++)
                for (int bits = 0; bits < 64; bits++)
                    for (int occ : occs)
                        for (int lstk : lstks) {
                            const bool nee = bits & 1, mis = bits & 2, count = bits & 4, moments = bits & 8, wave_ok = bits & 16, pixels_fit = bits & 32;
                            // skipped, each by a rule of ptmi.hip: PT_FLAG_MIS without PT_FLAG_NEE (pt_render's argument checks: PT_ERR_INVALID)
                            // and over Woop records (plan_call: PT_ERR_UNSUPPORTED); wave_ok with another walk or with a map (plan_call's wave_ok)
                            if ((mis && (!nee || walk == ALG_WIDE_WOOP)) || (wave_ok && (walk != ALG_WIDE || map != ENV_NONE))) continue;
                            CHECK(env_code(map != ENV_NONE, map == ENV_LIGHT) == map);
                            const int k = path_kernel(mis ? (int)PT_KERNEL_MEGA_BVH2 : kernel, walk, wave_ok, nee, pixels_fit);
                            if (k == PT_KERNEL_MEGA_BVH2) mega.request(mega_word(count, occ, lstk, walk, map, mis));
                            else if (k == PT_KERNEL_PERSISTENT) persist.request(persist_word(count, occ, lstk, walk, map));
                            else {
                                CHECK(k == PT_KERNEL_WAVEFRONT && wave_ok && !mis);
                                wave_calls.insert((count ? 1 : 0) | (nee ? 2 : 0) | (lstk == 24 ? 4 : 0) | (moments ? 8 : 0));
                            }
                        }
    CHECK(wave_calls.size() == 16);   // every combination the loop below starts from

    // render_wavefront: the plan of every such call (wave_plan), bounce by bounce at depths 1 .. 4.  (spp, sample group): one sample; the
    // groups of 4, 8 and 16 that a fused fold needs; a group that is not the whole call.  The history never holds under PT_FLAG_NEE.
    const uint32_t spps[][2] = {{1, 0}, {4, 2}, {8, 3}, {16, 4}, {32, 4}};
    for (int call : wave_calls)
        for (int bits = 0; bits < 64; bits++)
            for (int opts = 0; opts < 243; opts++)
                for (uint32_t depth = 1; depth <= 4; depth++)
                    for (const uint32_t* ss : spps) {
                        WaveRequest r = {};
                        r.count = call & 1; r.nee = call & 2; r.deep_stack = call & 4; r.moments = call & 8;
                        r.packet = bits & 1; r.anyhit_scene = bits & 2; r.history_holds = bits & 4; r.tree_has_occluders = bits & 8;
                        r.spp_fits_entry = bits & 16; r.fuse_stages = bits & 32 ? 1 : 0;
                        // skipped: path_history_holds (pt_ctx.h) is false for every call with PT_FLAG_NEE.  shade_word carries the plan's
                        // history into WS_HIST whatever nee says, and no NEE kernel has it: a looser path_history_holds has to show up HERE
                        if (r.history_holds && r.nee) continue;
                        r.last_anyhit = opts % 3; r.root_cull = opts / 3 % 3; r.root_entry = opts / 9 % 3; r.path_history = opts / 27 % 3;
                        r.last_occluders = opts / 81 % 3;
                        r.depth = depth; r.spp = ss[0]; r.sgroup_log2 = ss[1];
                        const WavePlan p = wave_plan_of(r);
                        for (uint32_t b = 0; b < depth; b++) {
                            const WaveExtend e = p.extend(b, depth);
                            if (e == EXT_FUSED) fused.request(fused_word(p, depth));
                            else if (e != EXT_PACKET) extend.request(extend_word(p, e));   // (k_wf_extend_packet has COUNT alone)
                            const WaveShade s = p.shade(b, depth);
                            CHECK((s == SHADE_NONE) == (e == EXT_FUSED));
                            if (s == SHADE_LAST_ANY) last_any.request(shade_word(p, s, b == 0));
                            else if (s != SHADE_NONE) shade.request(shade_word(p, s, b == 0));
                            if (r.nee) extend.request(extend_word(p, EXT_CLOSEST));   // the bounce's shadow rays
                        }
                    }

    // pt_render_rays: choose_walk without the postponed leaf (4 runs as 2); PT_FLAG_MIS as above
    for (int walk = ALG_WHILE; walk <= ALG_WIDE_WOOP; walk++)
        for (int map = ENV_NONE; map <= ENV_LIGHT; map++)
            for (int bits = 0; bits < 4; bits++) {
                const bool nee = bits & 1, mis = bits & 2;
                if (mis && (!nee || walk == ALG_WIDE_WOOP)) continue;   // (pt_render_rays' own checks refuse both: PT_ERR_INVALID, PT_ERR_UNSUPPORTED)
                rays.request(rays_word(walk, map, nee, mis));
            }
    // pt_closest_hits / pt_any_hits on a tree the wide walk fits: PT_OPT_LDS_STACK 0, 16, 24
    for (int any = 0; any < 2; any++)
        for (int lstk : {0, 16, 24}) query.request(query_word(any != 0, lstk == 24));

    for (const Family* f : {&mega, &persist, &rays, &query, &extend, &shade, &last_any, &fused}) f->report();
    // the budgets the words carry are the ones the requests asked for, or the nearest
    CHECK(budget_occ(mega_budget(6, 16)) == 8 && budget_occ(mega_budget(4, 16)) == 4 && budget_lstk(mega_budget(8, 72)) == 72);
    CHECK(persist_budget(ALG_WIDE, 5, 16) == BUDGET_6x16 && persist_budget(ALG_WIDE, 8, 24) == BUDGET_6x24 && persist_budget(ALG_UNIFIED, 4, 24) == BUDGET_8x16);
    CHECK(shade_env(ENV_LIGHT, false, false) == ENV_LOOKUP && shade_env(ENV_LOOKUP, true, true) == ENV_LIGHT && shade_env(ENV_LIGHT, true, false) == ENV_LIGHT);
    for (int lp : {0, 1, 2, 4}) CHECK(ws_fold(ws_fold_field(lp)) == lp);
    if (n_failed) {
        std::printf("%d checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("all checks hold\n");
    return 0;
}
