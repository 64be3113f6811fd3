// The stepper's scalar board: d_scalar (device) and its mapped mirror h_scalar (HipOptimizer, hip_ipc.h) hold one double per slot below, and
// h_scalar.p[S] is only ever the published copy of d_scalar.p[S].  A slot has one meaning.  Slots that come back together are neighbours, so that
// every read-back is one contiguous publish of at most one wave of 32-bit words.  Plain C++: host code and k_iter_reset include it.
#pragma once

namespace ipcgpu {

enum ScalarSlot : int {
    S_E_ITERATE = 0, // E at the iterate (elasticity + inertia).  Written by enqueueElasticEnergy; read by computeSearchDir's tails, lineSearch, beginTimestep, computeEnergyVal.  Live from that launch to the publish behind it.
    S_E_TRIAL, // E at the trial point of the fused first line-search trial.  Written by the fast path's second enqueueElasticEnergy; read with the fast path's publish.
    S_STEP_FILTER, // minimum of the inversion step filter.  Reset by k_iter_reset or launch_fill, written by launch_inversion_step; read by launch_trial_step_fused, stepBounds and filterStepSize.  Live across those launches.
    S_DIR_NORM, // |p|inf of the search direction.  Reset by k_iter_reset or enqueueDirNorm, written by launch_max_abs; read with the publish behind the solve or by readScalar.
    S_CONTACT_E, // barrier energy of the self-contact sets.  Written by HipContact::energyEnqueue, whose launch publishes S_E_ITERATE .. S_CONTACT_E; read by computeEnergyVal and ipcgpu_contact_energy.
    S_TRIAL_ALPHA, // step size the fused trial step decided on the device.  Written by launch_trial_step_fused; read with the publish of the fast path and of beginTimestep.
    S_FRICTION_E, // lagged friction energy of the self-contact set: the reduction target of HipContact::frictionEnergy, written and read inside that call.
    S_DAMPING_E, // lagged damping energy.  Written by dampingEnergy's launch_dot_scaled, read by the readScalar behind it.
    S_KAPPA_NUM, // initKappa's two dot products, written by one launch_dot2 and published together: barrier gradient . elastic gradient ...
    S_KAPPA_DEN, // ... and barrier gradient . barrier gradient
    S_INVERSION_SUM, // checkInversion on several processes: the flag as a double, uploaded from its own place in the mirror (pinned), all-reduced, read by readScalar.
    S_SCRATCH, // a value written and read inside one call: the Neumann energy per group, both MDBC reductions, the energies of the C entry points.
    S_COUNT
};

// The plastic flow's own two small boards (HipPlastic, hip_ipc.h; plastic_kernels.h): the stepper's launch adds to the integer one and never reads it on
// the fast path; ipcgpu_plastic_update and ipcgpu_plastic_state read them.
enum PlasticCount : int {
    PC_YIELDED = 0, // elements the last flow rewrote.  Zeroed before every flow, added to by k_plastic_flow (integer atomics).
    PC_SKIPPED, // elements the last flow found flat or inverted (s2 <= 0) and left alone
    PC_COUNT
};
enum PlasticTotal : int {
    PT_MAX_ALPHA = 0, // the largest accumulated plastic strain.  Written by launch_plastic_state's reduction, read by ipcgpu_plastic_state behind it.
    PT_VOL_ALPHA, // sum of rest volume times accumulated plastic strain
    PT_COUNT
};

// The shells' plastic flow keeps the same two boards (HipShellPlastic, hip_ipc.h; shell_plastic_kernels.h): the stepper's launches add to the integer one
// and never read it; ipcgpu_shell_plastic_update and ipcgpu_shell_plastic_state read them.
enum ShellPlasticCount : int {
    SPC_TRI_YIELDED = 0, // triangles the last flow rewrote.  Zeroed before every flow, added to by k_shell_plastic_flow_tri (integer atomics).
    SPC_TRI_SKIPPED, // triangles the last flow found collapsed (l2 <= 0 or not finite) and left alone.  (Stays behind SPC_TRI_YIELDED: the kernel adds to the pair.)
    SPC_HINGE_YIELDED, // hinges the last flow rewrote.  Added to by k_shell_plastic_flow_hinge.
    SPC_HINGE_SKIPPED, // hinges the last flow found with a zero-length n1, n2 or e and left alone.  (Stays behind SPC_HINGE_YIELDED.)
    SPC_COUNT
};
enum ShellPlasticTotal : int {
    SPT_MAX_ALPHA = 0, // the largest accumulated membrane plastic strain.  Written by launch_shell_plastic_state's reduction, read by ipcgpu_shell_plastic_state behind it.
    SPT_MAX_ALPHA_B, // the largest accumulated outer-fibre plastic strain of a hinge
    SPT_HA_ALPHA, // sum of rest volume h A times alpha over the triangles
    SPT_COUNT
};
static_assert(SPC_TRI_SKIPPED == SPC_TRI_YIELDED + 1 && SPC_HINGE_SKIPPED == SPC_HINGE_YIELDED + 1, "a flow kernel adds to a pair of neighbours");

// how many slots first .. last are: the count of a publish
constexpr int slotSpan(ScalarSlot first, ScalarSlot last) { return last - first + 1; }

// the fast path and beginTimestep read back S_E_ITERATE .. S_TRIAL_ALPHA, computeEnergyVal S_E_ITERATE .. S_CONTACT_E, the diagonal fallback S_E_ITERATE .. S_DIR_NORM
static_assert(S_E_ITERATE == 0 && S_E_TRIAL == 1 && S_STEP_FILTER == 2 && S_DIR_NORM == 3 && S_CONTACT_E == 4 && S_TRIAL_ALPHA == 5 && S_KAPPA_DEN == S_KAPPA_NUM + 1,
    "slots that are published together must stay neighbours");
static_assert(2 * S_COUNT <= 64, "the publish kernel runs one wave: one lane per 32-bit word");

} // namespace ipcgpu
