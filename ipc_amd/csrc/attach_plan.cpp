// Host side of the attachments: see attach_plan.h.  Host only.
#include "attach_plan.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>

namespace ipcgpu {

bool buildAttachPlan(int nV, int n, const int* nodesA, const double* weightsA, const int* nodesB, const double* weightsB, const double* k, const double* L,
    AttachPlan& plan, std::string& err)
{
    plan = AttachPlan();
    auto fail = [&](const std::string& what) {
        plan = AttachPlan();
        err = what;
        return false;
    };
    if (nV <= 0 || n < 0) return fail("set_attachments: bad sizes");
    if (n > 0 && (!nodesA || !weightsA || !nodesB || !weightsB || !k || !L)) return fail("set_attachments: null argument");
    if ((long long)n * ATTACH_SLOTS > 0x7fffffffLL) return fail("set_attachments: too many attachments");
    plan.n = n;
    if (n == 0) return true;
    const std::size_t N = (std::size_t)n;
    plan.count.assign(N, 0);
    plan.node.assign(ATTACH_SLOTS * N, 0);
    plan.coef.assign(ATTACH_SLOTS * N, 0.0);
    plan.kL.assign(2 * N, 0.0);
    std::vector<std::pair<int, int>> pairs;
    for (std::size_t i = 0; i < N; ++i) {
        const std::string at = "set_attachments: attachment " + std::to_string(i);
        if (!(k[i] > 0.0) || !std::isfinite(k[i])) return fail(at + " needs a finite stiffness k > 0");
        if (!(L[i] >= 0.0) || !std::isfinite(L[i])) return fail(at + " needs a finite rest length L >= 0");
        int ids[ATTACH_SLOTS];
        double c[ATTACH_SLOTS];
        int m = 0;
        for (int side = 0; side < 2; ++side) {
            const int* nodes = (side ? nodesB : nodesA) + 3 * i;
            const double* w = (side ? weightsB : weightsA) + 3 * i;
            const char* name = side ? "B" : "A";
            double sum = 0.0;
            int used = 0;
            for (int s = 0; s < 3; ++s) {
                if (!std::isfinite(w[s])) return fail(at + ": a weight of point " + name + " is not finite");
                if (w[s] < 0.0) return fail(at + ": a negative weight in point " + name);
                if (nodes[s] == -1) {
                    if (w[s] != 0.0) return fail(at + ": an unused slot of point " + name + " has a weight");
                    continue;
                }
                if (nodes[s] < 0 || nodes[s] >= nV) return fail(at + ": point " + name + " has a node id out of range");
                ++used;
                sum += w[s];
                const double signedW = side ? -w[s] : w[s];
                int j = 0;
                while (j < m && ids[j] != nodes[s]) ++j;
                if (j == m) {
                    ids[m] = nodes[s];
                    c[m] = 0.0;
                    ++m;
                }
                c[j] += signedW;
            }
            if (!used) return fail(at + ": point " + name + " has no node");
            if (!(std::fabs(sum - 1.0) <= 1e-12)) return fail(at + ": the weights of point " + name + " do not sum to 1");
        }
        int kept = 0;
        for (int j = 0; j < m; ++j)
            if (c[j] != 0.0) {
                ids[kept] = ids[j];
                c[kept] = c[j];
                ++kept;
            }
        // (the coefficients sum to 0 up to the tolerance above: fewer than two of them means the two points are one)
        if (kept < 2) return fail(at + " ties a point to itself (A and B are the same point)");
        plan.count[i] = kept;
        for (int s = 0; s < ATTACH_SLOTS; ++s) {
            plan.node[(std::size_t)s * N + i] = s < kept ? ids[s] : ids[0];
            plan.coef[(std::size_t)s * N + i] = s < kept ? c[s] : 0.0;
        }
        plan.kL[i] = k[i];
        plan.kL[N + i] = L[i];
        for (int a = 0; a < kept; ++a)
            for (int b = a + 1; b < kept; ++b) pairs.emplace_back(std::min(ids[a], ids[b]), std::max(ids[a], ids[b]));
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

double attachRestDistance(const AttachPlan& plan, int i, int nV, const double* Vrest)
{
    const std::size_t N = (std::size_t)plan.n, nv = (std::size_t)nV;
    double d[3] = { 0.0, 0.0, 0.0 };
    for (int s = 0; s < ATTACH_SLOTS; ++s) {
        const std::size_t v = (std::size_t)plan.node[(std::size_t)s * N + (std::size_t)i];
        const double c = plan.coef[(std::size_t)s * N + (std::size_t)i];
        for (int a = 0; a < 3; ++a) d[a] += c * Vrest[v + nv * a];
    }
    return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

} // namespace ipcgpu
