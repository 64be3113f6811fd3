// Host side of the fibre reinforcement of tetrahedral bodies (ipcgpu_set_fibers, ipcgpu_fiber_set_activation; fiber_kernels.hip): the per-element
// specification, kept current over calls that each set one contiguous range of elements (as ipcgpu_set_component_material; a later call overwrites,
// k == 0 removes), the activations per group, and the compact ascending lists the kernels read.  Pure host arithmetic (no HIP header:
// tests/test_fiber_plan_host.py builds it with g++).  The reference has no fibres; the model is stated in fiber_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

constexpr int FIBER_MAX_GROUPS = 64; // activation group ids are 0 .. FIBER_MAX_GROUPS - 1
enum FiberLaw : int { FIBER_LAW_SPRING = 0, FIBER_LAW_EXP = 1 };
enum FiberFlag : int { FIBER_FLAG_EXP = 1, FIBER_FLAG_TENSION_ONLY = 2 }; // the flag word of an element

struct FiberPlan {
    int nT = 0; // elements of the mesh the arrays belong to; 0: ipcgpu_set_fibers was never called
    // the specification, per element of the mesh
    std::vector<double> dir; // SoA [3][nT]: unit rest direction a (0 0 0 without a fibre)
    std::vector<double> k, k2; // nT: k == 0: no fibre; k2 is 0 under law 0
    std::vector<int> flags, group; // nT
    std::vector<double> act; // FIBER_MAX_GROUPS: activation per group, < 1
    // the compact lists (buildFiberLists), ascending in the element index
    int nF = 0;
    std::vector<int> fibTet, flagsF, groupOf; // nF
    std::vector<double> b; // SoA [3][nF]: A_t a
    std::vector<double> volK, k2F; // nF
    std::vector<double> l0; // FIBER_MAX_GROUPS: 1 - act
};

// Elements [tetBegin, tetEnd) of a mesh of nT elements get a fibre family: direction dir (3 doubles; with dirPerElement 3 per element of the range,
// element-major), stiffness k, law, k2 (read under law 1 only), tensionOnly (law 0; law 1 is always tension only), activation group.  The direction is
// normalised here.  k == 0 removes the fibres of the range (the other arguments are then not looked at, the range apart).  A plan of another nT (or an
// empty one) is first reset to "no fibre anywhere, every activation 0".  Changes the specification only: call buildFiberLists afterwards.
// false, with the reason in err and the plan as it was: nT <= 0; a range outside 0 <= tetBegin <= tetEnd <= nT; a null, zero or non-finite direction;
// k negative or not finite; a law other than 0 and 1; law 1 with k2 <= 0 or not finite; a group outside [0, FIBER_MAX_GROUPS); law 1 on a group
// whose activation is not 0.
bool setFiberRange(FiberPlan& plan, int nT, int tetBegin, int tetEnd, const double* dir, bool dirPerElement, double k, int law, double k2, bool tensionOnly,
    int group, std::string& err);
// The activation of one group: act < 1 and finite (negative: the fibres want to be longer).  false as above: a group out of range, act >= 1 or not
// finite, act != 0 on a group that holds a law-1 element.  Changes act and l0 and nothing per element.
bool setFiberActivation(FiberPlan& plan, int group, double act, std::string& err);
// The compact lists from the specification, the current restTriInv (SoA [9][nT], column-major inside the 9) and the rest volumes: b = A_t a, vol k.
// An element with vol k == 0 (a rest volume of 0) is left out.
void buildFiberLists(FiberPlan& plan, const double* restTriInv, const double* vol);

} // namespace ipcgpu
