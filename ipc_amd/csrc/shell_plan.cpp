// Host side of the elastic shells: see shell_plan.h.  Host only.
#include "shell_plan.h"
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace ipcgpu {

namespace {
inline void sub3(const double* a, const double* b, double* r)
{
    for (int i = 0; i < 3; ++i) r[i] = a[i] - b[i];
}
inline void cross3(const double* a, const double* b, double* r)
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

struct HalfEdge {
    int lo, hi, tri, opp;
    bool forward; // the triangle traverses lo -> hi
    bool operator<(const HalfEdge& o) const { return lo != o.lo ? lo < o.lo : (hi != o.hi ? hi < o.hi : tri < o.tri); }
};
} // namespace

double shellHingeAngle(const double x0[3], const double x1[3], const double x2[3], const double x3[3])
{
    double e[3], a[3], b[3], c[3], n1[3], n2[3], nn[3];
    sub3(x1, x0, e);
    sub3(x2, x0, a);
    cross3(e, a, n1);
    sub3(x0, x1, b);
    sub3(x3, x1, c);
    cross3(b, c, n2);
    cross3(n1, n2, nn);
    return std::atan2(dot3(nn, e) / std::sqrt(dot3(e, e)), dot3(n1, n2));
}

bool buildShellPlan(int nV, int nTri, const int* tri, const double* Vrest, const double* thickness, const double* YM, const double* PR, const double* rho,
    int nTet, const int* tets, ShellPlan& plan, std::string& err)
{
    plan = ShellPlan();
    auto fail = [&](const std::string& what) {
        plan = ShellPlan();
        err = what;
        return false;
    };
    if (nV <= 0 || nTri < 0 || nTet < 0) return fail("set_shell: bad sizes");
    if (nTri > 0 && (!tri || !Vrest || !thickness || !YM || !PR || !rho)) return fail("set_shell: null argument");
    if (nTet > 0 && !tets) return fail("set_shell: null tetrahedron list");
    if ((long long)nTri * 3 > 0x7fffffffLL) return fail("set_shell: too many triangles");
    plan.nTri = nTri;
    plan.mass.assign((std::size_t)nV, 0.0);
    plan.isShellNode.assign((std::size_t)nV, 0);
    if (nTri == 0) return true;
    const std::size_t nt = (std::size_t)nTri, nv = (std::size_t)nV;
    plan.tri.resize(3 * nt);
    plan.triConst.assign(6 * nt, 0.0);
    plan.area.assign(nt, 0.0);
    plan.membraneK.assign(nt, 0.0);
    plan.thickness.assign(nt, 0.0);
    std::vector<double> kb(nt);
    std::vector<HalfEdge> half;
    half.reserve(3 * nt);
    auto X = [&](int v, double* p) {
        for (int c = 0; c < 3; ++c) p[c] = Vrest[(std::size_t)v + nv * c];
    };
    for (std::size_t t = 0; t < nt; ++t) {
        int v[3];
        for (int k = 0; k < 3; ++k) {
            v[k] = tri[t + nt * k];
            if (v[k] < 0 || v[k] >= nV) return fail("set_shell: triangle " + std::to_string(t) + " has a node id out of range");
        }
        if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) return fail("set_shell: triangle " + std::to_string(t) + " repeats a node");
        const double h = thickness[t], E = YM[t], nu = PR[t], r = rho[t];
        if (!(h > 0.0) || !(E > 0.0) || !(r > 0.0) || !(nu > -1.0 && nu < 1.0))
            return fail("set_shell: triangle " + std::to_string(t) + " needs thickness > 0, E > 0, rho > 0 and -1 < nu < 1");
        double X0[3], X1[3], X2[3], u[3], w[3], n[3];
        X(v[0], X0);
        X(v[1], X1);
        X(v[2], X2);
        sub3(X1, X0, u);
        sub3(X2, X0, w);
        cross3(u, w, n);
        const double l = std::sqrt(dot3(u, u)), twoA = std::sqrt(dot3(n, n));
        if (!(l > 0.0) || !(twoA > 0.0) || !std::isfinite(twoA)) return fail("set_shell: triangle " + std::to_string(t) + " has zero rest area");
        const double p = dot3(w, u) / l, q = twoA / l; // Dm = [[l, p], [0, q]] in the frame (u / l, the in-plane normal of u)
        const double A = 0.5 * twoA;
        for (int k = 0; k < 3; ++k) plan.tri[3 * t + k] = v[k];
        plan.triConst[0 * nt + t] = 1.0 / l;
        plan.triConst[1 * nt + t] = 0.0;
        plan.triConst[2 * nt + t] = -p / (l * q);
        plan.triConst[3 * nt + t] = 1.0 / q;
        plan.triConst[4 * nt + t] = h * A * (E / (2.0 * (1.0 + nu)));
        plan.triConst[5 * nt + t] = h * A * (E * nu / (1.0 - nu * nu));
        plan.area[t] = A;
        plan.membraneK[t] = h * A * E;
        plan.thickness[t] = h;
        kb[t] = E * h * h * h / (24.0 * (1.0 - nu * nu));
        for (int k = 0; k < 3; ++k) {
            plan.mass[(std::size_t)v[k]] += r * h * A / 3.0;
            plan.isShellNode[(std::size_t)v[k]] = 1;
            const int a = v[k], b = v[(k + 1) % 3], o = v[(k + 2) % 3];
            half.push_back(HalfEdge{ std::min(a, b), std::max(a, b), (int)t, o, a < b });
            double Xa[3], Xb[3], d[3];
            X(a, Xa);
            X(b, Xb);
            sub3(Xb, Xa, d);
            plan.edgeLenSum += std::sqrt(dot3(d, d));
        }
    }
    for (std::size_t i = 0; i < 4 * (std::size_t)nTet; ++i) {
        if (tets[i] < 0 || tets[i] >= nV) return fail("set_shell: tetrahedron index out of range");
        if (plan.isShellNode[(std::size_t)tets[i]]) return fail("set_shell: shell node " + std::to_string(tets[i]) + " belongs to a tetrahedron");
    }
    std::sort(half.begin(), half.end());
    std::vector<std::pair<int, int>> pairs;
    pairs.reserve(half.size());
    for (std::size_t i = 0; i < half.size();) {
        std::size_t j = i + 1;
        while (j < half.size() && half[j].lo == half[i].lo && half[j].hi == half[i].hi) ++j;
        const HalfEdge& a = half[i];
        const std::string name = "(" + std::to_string(a.lo) + ", " + std::to_string(a.hi) + ")";
        if (j - i > 2) return fail("set_shell: edge " + name + " is shared by more than two triangles");
        pairs.emplace_back(a.lo, a.hi);
        if (j - i == 2) {
            const HalfEdge& b = half[i + 1];
            if (a.forward == b.forward) return fail("set_shell: the two triangles at edge " + name + " traverse it in the same direction (inconsistent orientation)");
            const HalfEdge& f = a.forward ? a : b;
            const HalfEdge& g = a.forward ? b : a;
            if (f.opp == g.opp) return fail("set_shell: the two triangles at edge " + name + " have the same three nodes");
            double x0[3], x1[3], x2[3], x3[3], e[3];
            X(a.lo, x0);
            X(a.hi, x1);
            X(f.opp, x2);
            X(g.opp, x3);
            sub3(x1, x0, e);
            plan.hinge.insert(plan.hinge.end(), { a.lo, a.hi, f.opp, g.opp });
            plan.restAngle.push_back(shellHingeAngle(x0, x1, x2, x3));
            plan.hingeWeight.push_back(3.0 * dot3(e, e) / (plan.area[(std::size_t)f.tri] + plan.area[(std::size_t)g.tri]));
            plan.hingeK.push_back(0.5 * (kb[(std::size_t)f.tri] + kb[(std::size_t)g.tri]));
            pairs.emplace_back(std::min(f.opp, g.opp), std::max(f.opp, g.opp));
        }
        i = j;
    }
    plan.nHinge = (int)plan.restAngle.size();
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
