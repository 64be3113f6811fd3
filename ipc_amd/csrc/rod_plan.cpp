// Host side of the elastic rods: see rod_plan.h.  Host only.
#include "rod_plan.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>

namespace ipcgpu {

namespace {
constexpr double PI = 3.14159265358979323846;
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
} // namespace

double rodCurvature(const double xa[3], const double xb[3], const double xc[3])
{
    double e0[3], e1[3];
    for (int i = 0; i < 3; ++i) {
        e0[i] = xb[i] - xa[i];
        e1[i] = xc[i] - xb[i];
    }
    const double p = std::sqrt(dot3(e0, e0) * dot3(e1, e1)), q = dot3(e0, e1), d = p + q;
    if (!(d > 0.0)) return std::numeric_limits<double>::infinity();
    return std::sqrt(4.0 * std::max(p - q, 0.0) / d); // (Cauchy-Schwarz: p >= q; the clamp only removes a rounding of a straight node)
}

bool buildRodPlan(int nV, int nSeg, const int* seg, const double* Vrest, const double* radius, const double* YM, const double* rho, int nTet, const int* tets,
    int nShellTri, const int* shellTri, RodPlan& plan, std::string& err)
{
    plan = RodPlan();
    auto fail = [&](const std::string& what) {
        plan = RodPlan();
        err = what;
        return false;
    };
    if (nV <= 0 || nSeg < 0 || nTet < 0 || nShellTri < 0) return fail("set_rod: bad sizes");
    if (nSeg > 0 && (!seg || !Vrest || !radius || !YM || !rho)) return fail("set_rod: null argument");
    if (nTet > 0 && !tets) return fail("set_rod: null tetrahedron list");
    if (nShellTri > 0 && !shellTri) return fail("set_rod: null shell triangle list");
    if ((long long)nSeg * 3 > 0x7fffffffLL) return fail("set_rod: too many segments");
    plan.nSeg = nSeg;
    plan.mass.assign((std::size_t)nV, 0.0);
    plan.isRodNode.assign((std::size_t)nV, 0);
    if (nSeg == 0) return true;
    const std::size_t ns = (std::size_t)nSeg, nv = (std::size_t)nV;
    plan.seg.resize(2 * ns);
    plan.segConst.assign(2 * ns, 0.0);
    auto X = [&](int v, double* p) {
        for (int c = 0; c < 3; ++c) p[c] = Vrest[(std::size_t)v + nv * c];
    };
    std::vector<std::pair<int, int>> keys; // (lo, hi) per segment: repeats in either direction
    keys.reserve(ns);
    std::vector<int> deg((std::size_t)nV, 0);
    for (std::size_t s = 0; s < ns; ++s) {
        const int a = seg[s], b = seg[s + ns];
        if (a < 0 || a >= nV || b < 0 || b >= nV) return fail("set_rod: segment " + std::to_string(s) + " has a node id out of range");
        if (a == b) return fail("set_rod: segment " + std::to_string(s) + " repeats a node");
        const double r = radius[s], E = YM[s], d = rho[s];
        if (!(r > 0.0) || !(E > 0.0) || !(d > 0.0)) return fail("set_rod: segment " + std::to_string(s) + " needs radius > 0, E > 0 and rho > 0");
        double Xa[3], Xb[3], e[3];
        X(a, Xa);
        X(b, Xb);
        for (int i = 0; i < 3; ++i) e[i] = Xb[i] - Xa[i];
        const double L = std::sqrt(dot3(e, e));
        if (!(L > 0.0) || !std::isfinite(L)) return fail("set_rod: segment " + std::to_string(s) + " has zero rest length");
        plan.seg[2 * s] = a;
        plan.seg[2 * s + 1] = b;
        plan.segConst[s] = L;
        plan.segConst[ns + s] = E * (PI * r * r) / L;
        plan.lenSum += L;
        const double half = d * (PI * r * r) * L / 2.0;
        plan.mass[(std::size_t)a] += half;
        plan.mass[(std::size_t)b] += half;
        plan.isRodNode[(std::size_t)a] = plan.isRodNode[(std::size_t)b] = 1;
        ++deg[(std::size_t)a];
        ++deg[(std::size_t)b];
        keys.emplace_back(std::min(a, b), std::max(a, b));
    }
    std::vector<std::pair<int, int>> pairs = keys;
    std::sort(pairs.begin(), pairs.end());
    for (std::size_t i = 0; i + 1 < pairs.size(); ++i)
        if (pairs[i] == pairs[i + 1])
            return fail("set_rod: segment (" + std::to_string(pairs[i].first) + ", " + std::to_string(pairs[i].second) + ") is repeated");
    for (std::size_t i = 0; i < 4 * (std::size_t)nTet; ++i) {
        if (tets[i] < 0 || tets[i] >= nV) return fail("set_rod: tetrahedron index out of range");
        if (plan.isRodNode[(std::size_t)tets[i]]) return fail("set_rod: rod node " + std::to_string(tets[i]) + " belongs to a tetrahedron");
    }
    for (std::size_t i = 0; i < 3 * (std::size_t)nShellTri; ++i) {
        if (shellTri[i] < 0 || shellTri[i] >= nV) return fail("set_rod: shell triangle index out of range");
        if (plan.isRodNode[(std::size_t)shellTri[i]]) return fail("set_rod: rod node " + std::to_string(shellTri[i]) + " belongs to a shell triangle");
    }
    // the two incident segments of every node of degree 2, in ascending segment order
    std::vector<int> first((std::size_t)nV, -1), second((std::size_t)nV, -1);
    for (std::size_t s = 0; s < ns; ++s)
        for (int k = 0; k < 2; ++k) {
            const std::size_t v = (std::size_t)plan.seg[2 * s + k];
            if (deg[v] != 2) continue;
            (first[v] < 0 ? first[v] : second[v]) = (int)s;
        }
    for (int b = 0; b < nV; ++b) {
        if (deg[(std::size_t)b] != 2) continue;
        const std::size_t s0 = (std::size_t)first[(std::size_t)b], s1 = (std::size_t)second[(std::size_t)b];
        const int a = plan.seg[2 * s0] == b ? plan.seg[2 * s0 + 1] : plan.seg[2 * s0];
        const int c = plan.seg[2 * s1] == b ? plan.seg[2 * s1 + 1] : plan.seg[2 * s1];
        const double Em = 0.5 * (YM[s0] + YM[s1]), rm = 0.5 * (radius[s0] + radius[s1]);
        double Xa[3], Xb[3], Xc[3];
        X(a, Xa);
        X(b, Xb);
        X(c, Xc);
        plan.bend.insert(plan.bend.end(), { a, b, c });
        plan.bendK.push_back(Em * (PI * rm * rm * rm * rm / 4.0) / (plan.segConst[s0] + plan.segConst[s1]));
        plan.restKb.push_back(rodCurvature(Xa, Xb, Xc));
        pairs.emplace_back(std::min(a, c), std::max(a, c)); // (a != c: a repeated segment was refused above)
    }
    plan.nBend = (int)plan.bendK.size();
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
