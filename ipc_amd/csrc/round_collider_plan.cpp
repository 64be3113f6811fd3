// Round collider: validation of the parameters and the shape record.  See round_collider_plan.h.  Host only.
#include "round_collider_plan.h"
#include <cmath>

namespace ipcgpu {

bool checkRoundColliderDHat(const RoundShape& s, double dHat, std::string& err)
{
    if (s.side < 0.0 && !(s.R * s.R > dHat)) {
        err = "round collider: a hollow sphere needs R^2 > dHat (no active vertex may sit at its centre)";
        return false;
    }
    err.clear();
    return true;
}

bool planRoundCollider(const double* p0, const double* p1, double R, int hollow, double dHat, RoundShape& out, std::string& err)
{
    auto fail = [&](const char* what) {
        err = what;
        return false;
    };
    if (!p0 || !p1) return fail("round collider: null end point");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(p0[c]) || !std::isfinite(p1[c])) return fail("round collider: an end point is not finite");
    if (!std::isfinite(R)) return fail("round collider: the radius is not finite");
    if (!(R > 0.0)) return fail("round collider: the radius must be positive");
    if (hollow != 0 && hollow != 1) return fail("round collider: hollow is 0 or 1");
    const bool sphere = p0[0] == p1[0] && p0[1] == p1[1] && p0[2] == p1[2];
    if (hollow && !sphere) return fail("round collider: only a sphere (p0 == p1) may be hollow");
    RoundShape s;
    double d[3], l2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        s.p0[c] = p0[c];
        s.p1[c] = p1[c];
        d[c] = p1[c] - p0[c];
        l2 += d[c] * d[c];
    }
    s.len = sphere ? 0.0 : std::sqrt(l2);
    if (!sphere && !(s.len > 0.0 && std::isfinite(s.len))) return fail("round collider: the segment's length is zero or not finite in double precision");
    for (int c = 0; c < 3; ++c) s.axis[c] = sphere ? 0.0 : d[c] / s.len;
    s.R = R;
    s.side = hollow ? -1.0 : 1.0;
    if (dHat > 0.0 && !checkRoundColliderDHat(s, dHat, err)) return false;
    out = s;
    err.clear();
    return true;
}

} // namespace ipcgpu
