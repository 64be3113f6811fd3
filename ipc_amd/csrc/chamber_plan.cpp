// Host side of the pressure chambers: see chamber_plan.h.  Host only.
#include "chamber_plan.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>

namespace ipcgpu {

namespace {
struct EdgeUse {
    int lo, hi, forward, tri; // forward: the triangle walks the edge from lo to hi
    bool operator<(const EdgeUse& o) const { return lo != o.lo ? lo < o.lo : hi != o.hi ? hi < o.hi : tri < o.tri; }
};
} // namespace

bool buildChamberPlan(int nV, const double* Vrest, int nCh, const int* triEnd, const int* tri, const double* pressure, ChamberPlan& plan, std::string& err)
{
    plan = ChamberPlan();
    auto fail = [&](const std::string& what) {
        plan = ChamberPlan();
        err = what;
        return false;
    };
    if (nV <= 0 || nCh < 0) return fail("set_chambers: bad sizes");
    if (nCh == 0) return true;
    if (!Vrest || !triEnd || !pressure) return fail("set_chambers: null argument");
    for (int c = 0; c < nCh; ++c) {
        const int begin = c ? triEnd[c - 1] : 0;
        if (triEnd[c] < begin) return fail("set_chambers: triEnd is not ascending at chamber " + std::to_string(c));
        if (triEnd[c] == begin) return fail("set_chambers: chamber " + std::to_string(c) + " is empty");
        if (!std::isfinite(pressure[c])) return fail("set_chambers: the pressure of chamber " + std::to_string(c) + " is not finite");
    }
    const int nTri = triEnd[nCh - 1];
    if (!tri) return fail("set_chambers: null argument");
    if ((long long)nTri * 3 > 0x7fffffffLL) return fail("set_chambers: too many triangles");
    const std::size_t N = (std::size_t)nTri, nv = (std::size_t)nV;
    plan.n = nCh;
    plan.nTri = nTri;
    plan.triEnd.assign(triEnd, triEnd + nCh);
    plan.pressure.assign(pressure, pressure + nCh);
    plan.tri.assign(tri, tri + 3 * N); // column-major nTri x 3 IS the SoA [3][nTri]
    plan.chamberOf.assign(N, 0);
    plan.restRef.assign(3 * (std::size_t)nCh, 0.0);
    plan.restVolume.assign((std::size_t)nCh, 0.0);
    std::vector<std::pair<int, int>> pairs;
    pairs.reserve(3 * N);
    std::vector<EdgeUse> uses;
    for (int c = 0; c < nCh; ++c) {
        const std::string at = "set_chambers: chamber " + std::to_string(c);
        const int begin = c ? triEnd[c - 1] : 0, end = triEnd[c];
        uses.clear();
        for (int t = begin; t < end; ++t) {
            const int v[3] = { tri[t], tri[N + t], tri[2 * N + t] };
            for (int k = 0; k < 3; ++k)
                if (v[k] < 0 || v[k] >= nV) return fail(at + ": triangle " + std::to_string(t) + " has a node id out of range");
            if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) return fail(at + ": triangle " + std::to_string(t) + " repeats a node");
            plan.chamberOf[t] = c;
            for (int k = 0; k < 3; ++k) {
                const int a = v[k], b = v[(k + 1) % 3];
                uses.push_back({ std::min(a, b), std::max(a, b), a < b ? 1 : 0, t });
                pairs.emplace_back(std::min(a, b), std::max(a, b));
            }
        }
        std::sort(uses.begin(), uses.end());
        for (std::size_t i = 0; i < uses.size();) {
            std::size_t j = i;
            while (j < uses.size() && uses[j].lo == uses[i].lo && uses[j].hi == uses[i].hi) ++j;
            const std::string edge = "edge (" + std::to_string(uses[i].lo) + ", " + std::to_string(uses[i].hi) + ")";
            if (j - i != 2) return fail(at + ": " + edge + " is used by " + std::to_string(j - i) + " of its triangles, not by two (the surface is not closed)");
            if (uses[i].forward == uses[i + 1].forward)
                return fail(at + ": triangles " + std::to_string(uses[i].tri) + " and " + std::to_string(uses[i + 1].tri) + " traverse " + edge + " in the same direction");
            i = j;
        }
        // the reference point and the volume at rest, in the order chamber_plan.h states
        double S[3] = { 0.0, 0.0, 0.0 };
        for (int t = begin; t < end; ++t)
            for (int a = 0; a < 3; ++a) S[a] += (Vrest[tri[t] + nv * a] + Vrest[tri[N + t] + nv * a]) + Vrest[tri[2 * N + t] + nv * a];
        const double m3 = 3.0 * (double)(end - begin);
        double r[3];
        for (int a = 0; a < 3; ++a) plan.restRef[3 * (std::size_t)c + a] = r[a] = S[a] / m3;
        double V6 = 0.0;
        for (int t = begin; t < end; ++t) {
            double y[3][3];
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) y[k][a] = Vrest[tri[k * N + t] + nv * a] - r[a];
            V6 += (y[0][0] * (y[1][1] * y[2][2] - y[1][2] * y[2][1]) + y[0][1] * (y[1][2] * y[2][0] - y[1][0] * y[2][2])) + y[0][2] * (y[1][0] * y[2][1] - y[1][1] * y[2][0]);
        }
        plan.restVolume[c] = V6 / 6.0;
        if (!(plan.restVolume[c] > 0.0))
            return fail(at + " has the rest volume " + std::to_string(plan.restVolume[c]) + " <= 0: its triangles are oriented inward (or it encloses nothing)");
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    plan.pairs.reserve(2 * pairs.size());
    for (const auto& p : pairs) {
        plan.pairs.push_back(p.first);
        plan.pairs.push_back(p.second);
    }
    return true;
}

bool chamberGasPressureOk(const ChamberGas& gas, int n, const double* pressure, std::string& err)
{
    if (!gas.nGas) return true;
    for (int c = 0; c < n; ++c)
        if (gas.isGas[c] && !(gas.ambient[c] + pressure[c] > 0.0)) {
            err = "gas chamber " + std::to_string(c) + ": ambient + pressure = " + std::to_string(gas.ambient[c] + pressure[c]) + " <= 0 (the absolute pressure at the fill volume must be positive)";
            return false;
        }
    return true;
}

bool buildChamberGas(const ChamberPlan& plan, const int* isGas, const double* ambient, const double* gamma, const double* fillVolume, ChamberGas& gas, std::string& err)
{
    gas = ChamberGas();
    auto fail = [&](const std::string& what) {
        gas = ChamberGas();
        err = what;
        return false;
    };
    const int n = plan.n;
    if (n <= 0) return fail("chamber_set_gas without chambers");
    if (!isGas || !ambient || !gamma) return fail("chamber_set_gas: null argument");
    gas.isGas.assign((std::size_t)n, 0);
    gas.ambient.assign((std::size_t)n, 0.0);
    gas.gamma.assign((std::size_t)n, 1.0);
    gas.fillVolume = plan.restVolume;
    for (int c = 0; c < n; ++c) {
        if (!isGas[c]) continue;
        const std::string at = "chamber_set_gas: chamber " + std::to_string(c);
        if (!std::isfinite(ambient[c]) || !std::isfinite(gamma[c]) || (fillVolume && !std::isfinite(fillVolume[c]))) return fail(at + " has a parameter that is not finite");
        if (ambient[c] < 0.0) return fail(at + " has the ambient pressure " + std::to_string(ambient[c]) + " < 0");
        if (gamma[c] < 1.0) return fail(at + " has the exponent gamma " + std::to_string(gamma[c]) + " < 1");
        gas.isGas[c] = 1;
        gas.ambient[c] = ambient[c];
        gas.gamma[c] = gamma[c];
        if (fillVolume && fillVolume[c] > 0.0) gas.fillVolume[c] = fillVolume[c];
        gas.gasChamber.push_back(c);
    }
    gas.nGas = (int)gas.gasChamber.size();
    if (gas.nGas > CHAMBER_GAS_MAX)
        return fail("chamber_set_gas: " + std::to_string(gas.nGas) + " gas chambers, more than the " + std::to_string(CHAMBER_GAS_MAX) + " a context can hold");
    std::string perr;
    if (!chamberGasPressureOk(gas, n, plan.pressure.data(), perr)) return fail("chamber_set_gas: " + perr);
    gas.sliceOff.push_back(0);
    for (int c : gas.gasChamber) {
        const int begin = c ? plan.triEnd[c - 1] : 0, end = plan.triEnd[c];
        for (int b = begin; b < end; b += CHAMBER_GAS_SLICE) {
            gas.sliceBegin.push_back(b);
            gas.sliceEnd.push_back(std::min(b + CHAMBER_GAS_SLICE, end));
        }
        gas.sliceOff.push_back(gas.nSlice());
    }
    return true;
}

} // namespace ipcgpu
