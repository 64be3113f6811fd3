// Round collider (ipcgpu_opt_add_round_collider): validation of the caller's parameters and the record the kernels take by value.  A round collider is
// a segment [p0, p1] with a radius R > 0: a sphere where p0 == p1, a capsule otherwise; a sphere may be hollow (the bodies live inside it).  A hollow
// capsule is refused.  Pure host logic (no HIP header: tests/test_round_collider_plan_host.py builds it with g++).  The model is stated in
// round_collider_kernels.h.
#pragma once
#include <string>

namespace ipcgpu {

struct RoundShape {
    double p0[3], p1[3];
    double axis[3]; // unit vector from p0 to p1; zero for a sphere
    double len;     // |p1 - p0|; 0 for a sphere
    double R;
    double side;    // +1 solid, -1 hollow
};

// dHat: the squared activation distance of the context (<= 0: not known yet, the rule that needs it is left to checkRoundColliderDHat).
// On success returns true and fills `out`; on failure returns false with the reason in err and leaves `out` alone.
bool planRoundCollider(const double* p0, const double* p1, double R, int hollow, double dHat, RoundShape& out, std::string& err);

// The rule that depends on dHat, asked again whenever dHat is set: a hollow sphere needs R^2 > dHat, so that no active vertex sits at its centre.
bool checkRoundColliderDHat(const RoundShape& s, double dHat, std::string& err);

} // namespace ipcgpu
