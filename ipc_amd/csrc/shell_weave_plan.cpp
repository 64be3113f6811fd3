// Host side of the shells' woven cloth: see shell_weave_plan.h.  Host only.
#include "shell_weave_plan.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <map>
#include <utility>

namespace ipcgpu {

namespace {
struct RestFrame {
    double t1[3], t2[3]; // orthonormal in the rest plane, t1 along X1 - X0, t2 towards X2 (the frame of ShellPlan::triConst)
};
RestFrame restFrame(const ShellPlan& shell, int nV, const double* Vrest, int t)
{
    const int* v = &shell.tri[3 * (std::size_t)t];
    double u[3], w[3];
    for (int c = 0; c < 3; ++c) {
        u[c] = Vrest[v[1] + (std::size_t)nV * c] - Vrest[v[0] + (std::size_t)nV * c];
        w[c] = Vrest[v[2] + (std::size_t)nV * c] - Vrest[v[0] + (std::size_t)nV * c];
    }
    RestFrame f;
    const double l = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int c = 0; c < 3; ++c) f.t1[c] = u[c] / l;
    const double p = w[0] * f.t1[0] + w[1] * f.t1[1] + w[2] * f.t1[2];
    double r[3];
    for (int c = 0; c < 3; ++c) r[c] = w[c] - p * f.t1[c];
    const double q = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int c = 0; c < 3; ++c) f.t2[c] = r[c] / q;
    return f;
}
} // namespace

bool buildShellWeavePlan(const ShellPlan& shell, int nV, const double* Vrest, const int* woven, const double* dir, const double* E1, const double* E2,
    const double* G12, const double* nu12, const double* bendWarp, const double* bendWeft, ShellWeavePlan& plan, std::string& err)
{
    plan = ShellWeavePlan();
    auto fail = [&](const std::string& what) {
        plan = ShellWeavePlan();
        err = what;
        return false;
    };
    const int nTri = shell.nTri;
    plan.nTri = nTri;
    if (!woven || nTri == 0) return true;
    const std::size_t nt = (std::size_t)nTri;
    for (std::size_t t = 0; t < nt; ++t)
        if (woven[t] != 0 && woven[t] != 1) return fail("shell_set_weave: triangle " + std::to_string(t) + " has a selector other than 0 or 1");
    if (std::none_of(woven, woven + nt, [](int w) { return w == 1; })) return true;
    if (!dir || !E1 || !E2 || !G12 || !Vrest) return fail("shell_set_weave: null argument");
    std::vector<double> rows[6], bw(nt, 1.0), bf(nt, 1.0);
    std::vector<double> a(2 * nt, 0.0), const4(4 * nt, 0.0);
    for (std::size_t t = 0; t < nt; ++t) {
        if (!woven[t]) continue;
        const std::string name = "shell_set_weave: triangle " + std::to_string(t);
        const double d[3] = { dir[3 * t], dir[3 * t + 1], dir[3 * t + 2] };
        const double e1 = E1[t], e2 = E2[t], g = G12[t], nu = nu12 ? nu12[t] : 0.0, kw = bendWarp ? bendWarp[t] : 1.0, kf = bendWeft ? bendWeft[t] : 1.0;
        for (double v : { d[0], d[1], d[2], e1, e2, g, nu, kw, kf })
            if (!std::isfinite(v)) return fail(name + " has a value that is not finite");
        if (!(e1 > 0.0) || !(e2 > 0.0) || !(g > 0.0)) return fail(name + " has a modulus E1, E2 or G12 that is not positive");
        if (!(nu * nu < e1 / e2)) return fail(name + " has nu12^2 >= E1 / E2: the law is not positive definite");
        if (!(kw > 0.0) || !(kf > 0.0)) return fail(name + " has a bend factor that is not positive");
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 0.0)) return fail(name + " has a direction of zero length");
        const RestFrame f = restFrame(shell, nV, Vrest, (int)t);
        // (on the normalised direction: a long or a short vector names the same direction)
        const double ax = (d[0] / len) * f.t1[0] + (d[1] / len) * f.t1[1] + (d[2] / len) * f.t1[2];
        const double ay = (d[0] / len) * f.t2[0] + (d[1] / len) * f.t2[1] + (d[2] / len) * f.t2[2];
        const double pl = std::sqrt(ax * ax + ay * ay);
        if (!(pl >= 1e-6)) return fail(name + " has a direction normal to the triangle (its projection into the rest plane is shorter than 1e-6 of its length)");
        const double hA = shell.thickness[t] * shell.area[t];
        const double nu21 = nu * e2 / e1, den = 1.0 - nu * nu21;
        const double c4[4] = { e1 / den, nu * e2 / den, e2 / den, g };
        plan.tri.push_back((int)t);
        a[2 * t] = ax / pl;
        a[2 * t + 1] = ay / pl;
        rows[0].push_back(a[2 * t]);
        rows[1].push_back(a[2 * t + 1]);
        for (int k = 0; k < 4; ++k) {
            const4[4 * t + k] = c4[k];
            rows[2 + k].push_back(hA * c4[k]);
        }
        bw[t] = kw;
        bf[t] = kf;
    }
    plan.nWoven = (int)plan.tri.size();
    for (auto& r : rows) plan.wovConst.insert(plan.wovConst.end(), r.begin(), r.end());
    plan.woven.assign(woven, woven + nt);
    plan.a = std::move(a);
    plan.const4 = std::move(const4);
    // the hinges: the triangle opposite x2 traverses x0 -> x1, the one opposite x3 x1 -> x0 (shell_plan.h)
    std::map<std::pair<int, int>, int> triOfEdge; // directed edge -> its triangle
    for (int t = 0; t < nTri; ++t)
        for (int k = 0; k < 3; ++k) triOfEdge[{ shell.tri[3 * (std::size_t)t + k], shell.tri[3 * (std::size_t)t + (k + 1) % 3] }] = t;
    plan.hingeFactor.assign((std::size_t)shell.nHinge, 1.0);
    for (int i = 0; i < shell.nHinge; ++i) {
        const int x0 = shell.hinge[4 * (std::size_t)i], x1 = shell.hinge[4 * (std::size_t)i + 1];
        double e[3];
        for (int c = 0; c < 3; ++c) e[c] = Vrest[x1 + (std::size_t)nV * c] - Vrest[x0 + (std::size_t)nV * c];
        const double le2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
        double sum = 0.0;
        for (const std::pair<int, int>& key : { std::make_pair(x0, x1), std::make_pair(x1, x0) }) {
            const auto it = triOfEdge.find(key);
            const int t = it == triOfEdge.end() ? -1 : it->second;
            if (t < 0 || !woven[t]) {
                sum += 1.0;
                continue;
            }
            const RestFrame f = restFrame(shell, nV, Vrest, t);
            const double ex = e[0] * f.t1[0] + e[1] * f.t1[1] + e[2] * f.t1[2], ey = e[0] * f.t2[0] + e[1] * f.t2[1] + e[2] * f.t2[2];
            const double along = ex * plan.a[2 * (std::size_t)t] + ey * plan.a[2 * (std::size_t)t + 1];
            const double sin2 = std::min(1.0, std::max(0.0, 1.0 - along * along / le2));
            sum += bf[(std::size_t)t] + (bw[(std::size_t)t] - bf[(std::size_t)t]) * sin2;
        }
        plan.hingeFactor[(std::size_t)i] = 0.5 * sum;
    }
    return true;
}

std::vector<double> shellTriConstWithoutWeave(const std::vector<double>& triConst, const ShellWeavePlan& plan)
{
    std::vector<double> c = triConst;
    const std::size_t nt = (std::size_t)plan.nTri;
    if (c.size() != 6 * nt) return c;
    for (int t : plan.tri) c[4 * nt + (std::size_t)t] = c[5 * nt + (std::size_t)t] = 0.0;
    return c;
}

std::vector<double> shellHingeStiffnessWithWeave(const ShellPlan& shell, double bendScale, const ShellWeavePlan& plan)
{
    std::vector<double> k((std::size_t)shell.nHinge);
    const bool on = plan.nWoven > 0 && plan.hingeFactor.size() == k.size();
    for (std::size_t i = 0; i < k.size(); ++i) {
        k[i] = bendScale * shell.hingeK[i] * shell.hingeWeight[i];
        if (on) k[i] *= plan.hingeFactor[i];
    }
    return k;
}

} // namespace ipcgpu
