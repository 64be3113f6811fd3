// Host side of the aerodynamic surfaces: see aero_plan.h.  Host only.
#include "aero_plan.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <utility>

namespace ipcgpu {

void aeroRecord(const double* x0, const double* x1, const double* x2, double* rec)
{
    double e1[3], e2[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = x1[a] - x0[a];
        e2[a] = x2[a] - x0[a];
    }
    const double m[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    const double l = std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const bool ok = l > 0.0 && std::isfinite(l);
    for (int a = 0; a < 3; ++a) {
        rec[a] = ok ? m[a] / l : 0.0;
        rec[4 + a] = ((x0[a] + x1[a]) + x2[a]) / 3.0;
    }
    rec[3] = ok ? 0.5 * l : 0.0;
    rec[7] = 0.0;
}

bool buildAeroPlan(int nV, const double* Vrest, int nSurf, const int* triEnd, const int* tri, const double* cn, const double* ct, const int* oneSided, AeroPlan& plan,
    std::string& err)
{
    plan = AeroPlan();
    auto fail = [&](const std::string& what) {
        plan = AeroPlan();
        err = what;
        return false;
    };
    if (nV <= 0 || nSurf < 0) return fail("set_aero: bad sizes");
    if (nSurf == 0) return true;
    if (!Vrest || !triEnd || !cn || !ct || !oneSided) return fail("set_aero: null argument");
    for (int s = 0; s < nSurf; ++s) {
        const std::string at = "set_aero: surface " + std::to_string(s);
        const int begin = s ? triEnd[s - 1] : 0;
        if (triEnd[s] < begin) return fail("set_aero: triEnd is not ascending at surface " + std::to_string(s));
        if (triEnd[s] == begin) return fail(at + " is empty");
        if (!std::isfinite(cn[s]) || !std::isfinite(ct[s])) return fail(at + " has a coefficient that is not finite");
        if (cn[s] < 0.0 || ct[s] < 0.0) return fail(at + " has a negative coefficient");
    }
    const int nTri = triEnd[nSurf - 1];
    if (!tri) return fail("set_aero: null argument");
    if ((long long)nTri * 8 > 0x7fffffffLL) return fail("set_aero: too many triangles");
    const std::size_t N = (std::size_t)nTri, nv = (std::size_t)nV;
    plan.n = nSurf;
    plan.nTri = nTri;
    plan.triEnd.assign(triEnd, triEnd + nSurf);
    plan.tri.assign(tri, tri + 3 * N); // column-major nTri x 3 IS the SoA [3][nTri]
    plan.surfOf.assign(N, 0);
    plan.cn.assign(cn, cn + nSurf);
    plan.ct.assign(ct, ct + nSurf);
    plan.oneSided.assign((std::size_t)nSurf, 0);
    plan.coef.assign(4 * (std::size_t)nSurf, 0.0);
    plan.restRecord.assign(8 * N, 0.0);
    std::vector<std::pair<int, int>> pairs;
    pairs.reserve(3 * N);
    std::vector<std::array<int, 4>> keys; // sorted node ids, triangle
    keys.reserve(N);
    for (int s = 0; s < nSurf; ++s) {
        const std::string at = "set_aero: surface " + std::to_string(s);
        plan.oneSided[s] = oneSided[s] ? 1 : 0;
        plan.coef[4 * (std::size_t)s] = cn[s];
        plan.coef[4 * (std::size_t)s + 1] = ct[s];
        plan.coef[4 * (std::size_t)s + 2] = oneSided[s] ? 1.0 : 0.0;
        for (int t = s ? triEnd[s - 1] : 0; t < triEnd[s]; ++t) {
            const int v[3] = { tri[t], tri[N + t], tri[2 * N + t] };
            for (int k = 0; k < 3; ++k)
                if (v[k] < 0 || v[k] >= nV) return fail(at + ": triangle " + std::to_string(t) + " has a node id out of range");
            if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) return fail(at + ": triangle " + std::to_string(t) + " repeats a node");
            plan.surfOf[t] = s;
            double x[3][3];
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) x[k][a] = Vrest[v[k] + nv * a];
            double* rec = &plan.restRecord[8 * (std::size_t)t];
            aeroRecord(x[0], x[1], x[2], rec);
            if (!(rec[3] > 0.0)) return fail(at + ": triangle " + std::to_string(t) + " has zero rest area");
            std::array<int, 4> key = { v[0], v[1], v[2], t };
            std::sort(key.begin(), key.begin() + 3);
            keys.push_back(key);
            for (int k = 0; k < 3; ++k) {
                const int a = v[k], b = v[(k + 1) % 3];
                pairs.emplace_back(std::min(a, b), std::max(a, b));
            }
        }
    }
    std::sort(keys.begin(), keys.end());
    for (std::size_t i = 1; i < keys.size(); ++i)
        if (keys[i][0] == keys[i - 1][0] && keys[i][1] == keys[i - 1][1] && keys[i][2] == keys[i - 1][2])
            return fail("set_aero: surface " + std::to_string(plan.surfOf[keys[i][3]]) + ": triangle " + std::to_string(keys[i][3]) + " is listed twice (it is triangle "
                + std::to_string(keys[i - 1][3]) + " in another rotation or orientation)");
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    plan.pairs.reserve(2 * pairs.size());
    for (const auto& p : pairs) {
        plan.pairs.push_back(p.first);
        plan.pairs.push_back(p.second);
    }
    return true;
}

} // namespace ipcgpu
