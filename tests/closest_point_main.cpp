// closest_point_main.cpp -- nero_amd/csrc/closest_point_math.h, the source the closest-point kernel compiles, as a stand-alone host program
// (tests/test_closest_point_cpu.py builds and runs it under the sanitizers through tests.helpers.run_host_program).  For a fixed table of
// (point, triangle) pairs it prints one line per pair, every number as a hex float: the inputs p, v0, e1, e2 and the triangle's box mn, mx, then d2, b1,
// b2 of point_triangle, then box_bound of p against that box with CP_PAD and with no pad.  The test recomputes the outputs from the
// printed inputs with tests/closest_ref.py and compares bit for bit.
#include <cstdio>
#include <cmath>
#include <vector>

#include "../nero_amd/csrc/closest_point_math.h"

struct Tri3 { float v0[3], v1[3], v2[3]; };

int main() {
    const float third = 1.0f / 3.0f;
    const std::vector<Tri3> tris = {
        {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}},                                     // right triangle in z = 0
        {{0.1f, -0.2f, 0.3f}, {0.7f, 0.1f, -0.4f}, {-0.3f, 0.9f, 0.2f}},                         // general position
        {{0.25f, 0.25f, 0.25f}, {0.25f, 0.25f, 0.25f}, {0.25f, 0.25f, 0.25f}},                   // zero area: a point
        {{0.25f, 0.25f, 0.25f}, {0.25f, 0.25f, 0.25f}, {-0.5f, 0.75f, 0.125f}},                  // zero area: a repeated corner (e1 = 0)
        {{-0.5f, 0.75f, 0.125f}, {0.25f, 0.25f, 0.25f}, {-0.5f, 0.75f, 0.125f}},                 // zero area: a repeated corner (e2 = 0)
        {{0.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {1.f, 1.f, 1.f}},                                  // zero area: three collinear corners
        {{-1.f, 0.5f, 0.f}, {0.f, 0.5f + 1e-4f, 0.f}, {1.f, 0.5f, 0.f}},                         // a sliver of aspect 1e4
        {{1e-3f, 0.f, 0.f}, {1e-3f + 1e-6f, 0.f, 0.f}, {1e-3f, 1e-6f, 0.f}},                     // tiny
        {{third, -third, third}, {third + 0.1f, third, -0.3f}, {-third, 0.7f, third}},           // coordinates that are no short binary fractions
    };
    const float points[][3] = {
        {0.f, 0.f, 0.f}, {0.25f, 0.25f, 0.25f}, {0.25f, 0.25f, 0.f}, {0.5f, 0.5f, 0.f}, {0.5f, 0.f, 0.f}, {2.f, 2.f, 0.f}, {0.2f, 0.3f, 0.7f},
        {-1.f, -1.f, -1.f}, {0.3f, -0.4f, 0.f}, {9.5f, -8.25f, 7.f}, {1e-3f, 0.f, 0.f}, {third, third, third}, {-0.f, 0.f, -0.f},
    };
    using namespace nero_closest;
    for (const Tri3& t : tris) {
        float e1[3], e2[3], mn[3], mx[3];
        for (int k = 0; k < 3; ++k) {
            e1[k] = t.v1[k] - t.v0[k];
            e2[k] = t.v2[k] - t.v0[k];
            mn[k] = fminf(t.v0[k], fminf(t.v1[k], t.v2[k]));
            mx[k] = fmaxf(t.v0[k], fmaxf(t.v1[k], t.v2[k]));
        }
        std::vector<std::vector<float>> ps;
        for (const auto& p : points) ps.push_back({p[0], p[1], p[2]});
        // on the triangle itself: its corners, an edge midpoint, a point of its plane inside it and one of its plane outside it
        ps.push_back({t.v0[0], t.v0[1], t.v0[2]});
        ps.push_back({t.v1[0], t.v1[1], t.v1[2]});
        ps.push_back({t.v2[0], t.v2[1], t.v2[2]});
        ps.push_back({t.v0[0] + 0.5f * e1[0], t.v0[1] + 0.5f * e1[1], t.v0[2] + 0.5f * e1[2]});
        ps.push_back({t.v0[0] + 0.25f * e1[0] + 0.5f * e2[0], t.v0[1] + 0.25f * e1[1] + 0.5f * e2[1], t.v0[2] + 0.25f * e1[2] + 0.5f * e2[2]});
        ps.push_back({t.v0[0] - 0.75f * e1[0] + 2.f * e2[0], t.v0[1] - 0.75f * e1[1] + 2.f * e2[1], t.v0[2] - 0.75f * e1[2] + 2.f * e2[2]});
        for (const auto& p : ps) {
            const PointTri r = point_triangle(p.data(), t.v0, e1, e2);
            const float row[23] = {p[0], p[1], p[2], t.v0[0], t.v0[1], t.v0[2], e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], mn[0], mn[1], mn[2],
                                   mx[0], mx[1], mx[2], r.d2, r.b1, r.b2, box_bound(mn, mx, p.data(), CP_PAD), box_bound(mn, mx, p.data(), 0.f)};
            for (int k = 0; k < 23; ++k) std::printf("%a%c", row[k], k == 22 ? '\n' : ' ');
        }
    }
    return 0;
}
