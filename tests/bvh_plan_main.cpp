// Stand-alone host program over nero_amd/csrc/bvh_build_plan.h (no HIP): prints, for every nT in [first, last], the plan of the device BVH
// build -- header, level table, and per level what the walk range_of() gives for every range -- and the workspace carving's checks.
// tests/test_bvh_build_cpu.py builds it with the address and undefined-behaviour sanitizers and compares the lines with the numpy
// restatement's (tests/bvh_build_ref.py: plan_line).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../nero_amd/csrc/bvh_build_plan.h"

using namespace nero_bvh_plan;

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s first last lds_capacity\n", argv[0]); return 2; }
    const int first = atoi(argv[1]), last = atoi(argv[2]), cap = atoi(argv[3]);
    for (int nT = first; nT <= last; ++nT) {
        Plan p;
        if (!make_plan(nT, cap, &p)) { printf("%d refused\n", nT); continue; }
        printf("%d %d %d %d %d |", p.nT, p.n_nodes, p.n_levels, p.root, p.hand_off);
        for (int l = 0; l < p.n_table; ++l) printf(" %d:%d:%d", p.lv[l].a, p.lv[l].ia, p.lv[l].ib);
        printf(" |");
        std::vector<char> covered((size_t)nT, 0);
        for (int l = 0; l <= p.n_levels; ++l) {
            long long cnt = 0, inner = 0, sum_lo = 0, sum_n = 0, sum_node = 0;
            for (int k = 0; k < (1 << l); ++k) {
                const Range r = range_of(p, l, k);
                if (!r.valid) continue;
                ++cnt; sum_lo += r.lo; sum_n += r.n;
                if (r.n > LEAF_MAX) { ++inner; sum_node += r.node; }
                // locate() must find this range from its first and its last position
                int lo, n, lev;
                const int k0 = locate(nT, l, r.lo, &lo, &n, &lev), k1 = locate(nT, l, r.lo + r.n - 1, &lo, &n, &lev);
                if (k0 != k || k1 != k || lo != r.lo || n != r.n || lev != l) { printf(" LOCATE-MISMATCH"); return 1; }
                if (r.n <= LEAF_MAX)
                    for (int i = r.lo; i < r.lo + r.n; ++i) covered[(size_t)i]++;
            }
            printf(" %lld:%lld:%lld:%lld:%lld", cnt, inner, sum_lo, sum_n, sum_node);
        }
        for (int i = 0; i < nT; ++i)
            if (covered[(size_t)i] != 1) { printf(" LEAVES-DO-NOT-PARTITION"); return 1; }
        const Layout L = layout(p);
        if (L.temp + L.temp_bytes + 256 > L.total || L.heap_boxes < ((size_t)2 << p.n_levels) || L.ext_ranges * 2 < ((size_t)1 << p.hand_off))
            { printf(" LAYOUT"); return 1; }
        printf("\n");
    }
    return 0;
}
