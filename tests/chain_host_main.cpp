// stand-alone program over the planner of nero_amd/csrc/chain_host.h (no device code, no HIP runtime call): the C++ twin of
// nero_amd/chain.py::Chain on dry arenas, built by tests/test_chain_host_cpu.py with the host compiler and
// -fsanitize=address,undefined.  Every library entry point the planner would launch is a stub that aborts: a dry run reaches none.
// Output, per chain:  "chain <name> pack_floats <n> jobs <m>",  one "job <name> <entry> kind nrows ld col0 ncols transpose kpad nt_count
// scale" per pack job,  one "peak <name> <rows> <bytes>" per row count (dry forward(save) + backward(d_init, d_aux) + weight_grads);
// then "offsets <floats> ..." (where carve_chains puts each chain) and "total <floats>".
#define __HIP_PLATFORM_AMD__ 1
#include <cstdio>
#include <cstdlib>
#include "../nero_amd/csrc/chain_host.h"

static int reached(const char* what) {
    std::fprintf(stderr, "chain_host_main: %s reached from a dry run\n", what);
    std::abort();
}
int nero_fail(int, const char*) { return reached("nero_fail"); }
int nero_check_launch(const char*) { return reached("nero_check_launch"); }
extern "C" {
int nero_mlp_forward(const nero_fwd_chain*, int, void*) { return reached("nero_mlp_forward"); }
int nero_mlp_backward(const nero_bwd_chain*, int, void*) { return reached("nero_mlp_backward"); }
int nero_head_dw_ld(const float*, const float*, const float*, int, int, float*, int, int, float*, float*, int, void*) { return reached("nero_head_dw_ld"); }
int nero_dw_gemm_batch(const nero_dw_job*, int, int, float*, void*) { return reached("nero_dw_gemm_batch"); }
int nero_pack_batch(const nero_pack_job*, int, void*) { return reached("nero_pack_batch"); }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { reached("hipMemsetAsync"); return hipSuccess; }
}

int main() {
    // linear i of a chain: W = w + 16 i, b = w + 16 i + 8 (never followed: the entry of a pack job is read back from its source pointer)
    static float w[16 * 16];
    nero_linear L[16];
    nero_linear_grad G[16];
    for (int i = 0; i < 16; ++i) { L[i].W = w + 16 * i; L[i].b = w + 16 * i + 8; G[i].dW = w + 16 * i; G[i].db = w + 16 * i + 8; }
    Chain feats;                                   // the Stage-II feature chain of stage2_driver.hip::build_chains
    for (int i = 0; i < 8; ++i) {
        if (i == 0) feats.e.push_back(dense(L[0], 51, 256, NERO_ACT_RELU, 51));
        else if (i == 4) feats.e.push_back(dense(L[4], 307, 256, NERO_ACT_RELU, 256, 0, 51, 256));
        else feats.e.push_back(dense(L[i], 256, 256, i == 7 ? NERO_ACT_NONE : NERO_ACT_RELU, 256));
    }
    feats.k_init = 56; feats.k_aux = 56; feats.aux_wide = 1;
    struct Case { const char* name; Chain c; } cases[3] = {
        {"predictor", predictor(L, 256, 3, 256, 8, 3)}, {"predictor_no_aux", predictor(L, 123, 0, 128, 0, 3)}, {"feats", feats}};
    predictor_grads(cases[0].c, G, 259);
    predictor_grads(cases[1].c, G, 123);
    for (int i = 0; i < 8; ++i) set_dense_grad(cases[2].c.e[i], G[i], i == 0 ? 51 : (i == 4 ? 307 : 256));

    std::vector<Chain*> chains;
    for (Case& k : cases) chains.push_back(&k.c);
    const size_t total = pack_floats_total(chains);
    std::vector<float> buf(total);
    std::vector<nero_pack_job> all;
    carve_chains(chains, buf.data(), all);
    std::vector<ptrdiff_t> starts;                 // (a chain's first image is the bias image of its first entry)
    for (const Case& k : cases) starts.push_back(k.c.e[0].bias - buf.data());

    const Modes M = {NERO_GEMM_F16X3, NERO_GEMM_F16X3, NERO_GEMM_F16X3, NERO_GEMM_F16X3};
    const int rows[5] = {1, 63, 64, 65, 4097};
    float* const token = reinterpret_cast<float*>(0x1000);
    for (Case& k : cases) {
        Chain& c = k.c;
        std::vector<float> own(c.pack_floats());
        std::vector<nero_pack_job> jobs;
        float* q = own.data();
        c.pack(q, jobs);
        if (q != own.data() + own.size()) { std::fprintf(stderr, "%s: pack carved %td floats, pack_floats says %zu\n", k.name, q - own.data(), own.size()); return 1; }
        std::printf("chain %s pack_floats %zu jobs %zu\n", k.name, c.pack_floats(), jobs.size());
        for (const nero_pack_job& j : jobs)
            std::printf("job %s %d %d %d %d %d %d %d %d %d %.9g\n", k.name, (int)((j.W - w) / 16), j.kind, j.nrows, j.ld, j.col0, j.ncols, j.transpose, j.kpad,
                        j.nt_count, (double)j.scale);
        const bool ends_dense = c.e[c.n() - 1].d.has;
        for (const int n : rows) {
            Arena A;
            A.dry = true;
            Fwd F;
            Bwd B;
            const float* hd[MAXL] = {};
            if (!ends_dense) hd[c.n() - 1] = token;
            if (c.forward(A, M, token, c.k_init, c.k_aux ? token : nullptr, c.k_aux, n, true, F, nullptr) != NERO_OK) return 1;
            if (c.backward(A, M, F, n, ends_dense ? token : nullptr, ends_dense ? NERO_HID : 0, hd, true, true, nullptr, nullptr, 0, false, false, B,
                           nullptr) != NERO_OK)
                return 1;
            const size_t peak = A.peak;
            if (c.weight_grads(A, M, F, B, n, token, c.k_init, token, c.k_aux, hd, nullptr, nullptr, token, nullptr) != NERO_OK) return 1;
            if (A.failed || A.peak != peak) { std::fprintf(stderr, "%s: a dry arena failed, or weight_grads carved\n", k.name); return 1; }
            std::printf("peak %s %d %zu\n", k.name, n, peak);
        }
    }
    std::printf("offsets");
    for (const ptrdiff_t s : starts) std::printf(" %td", s);
    std::printf("\ntotal %zu jobs %zu\n", total, all.size());
    return 0;
}
