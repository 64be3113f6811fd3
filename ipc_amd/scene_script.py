"""The reference's scene-script grammar (src/Config.cpp:97-620) mapped onto the C ABI.

This is tooling, not product: a maintainer who links libipcgpu.so into IPC keeps IPC's own Config class; this module lets
the tests and tools/run_scene.py drive the library (or the CPU oracle, through the same `Backend` protocol) from the very
scene files the reference ships, so both start from identical inputs.  Only keywords whose feature exists here are accepted;
anything else raises `UnsupportedKeyword` instead of being ignored silently.

    cfg = SceneConfig.parse(open(path).read(), base_dir)       # grammar only
    scene = assemble(cfg, read_mesh)                          # shapes -> one mesh (main.cpp:880-1198); the script's set-up: anim_script.py
    apply(scene, backend)                                     # C-ABI calls, in the order INTEGRATION.md gives

Keywords of this project beside the reference's: `shell`, `limit`, `rod`, `contactGroup` on a shape line (see Shape), and the top-level lines
`contactIgnore`, `contactFric`, `attach <shapeA> <nodeA> <shapeB> <nodeB> <k> [<L>]` and `stitch <shapeA> <shapeB> <radius> <k> [rest]` (see SceneConfig):
the last two tie nodes of two shapes by springs (Context.set_attachments); barycentric points stay an API feature.  `pressure <p> [ramp <seconds>]
[gas <ambient> [gamma <g>]]` on a shape line (a `shell` shape or a tetrahedral shape) makes the shape's closed surface one pressure chamber, constant or
following the ideal-gas law (Context.set_chambers, Context.chamber_set_gas; see Shape).  `aero [cn <C>] [ct <C>] [onesided]` on such a shape line makes its
surface an aerodynamic surface (Context.set_aero; see Shape) in the wind of the top-level line `wind <wx> <wy> <wz> [density <rho>]` (see SceneConfig).
"""
from dataclasses import dataclass, field
import math
import os
import warnings

import numpy as np

from . import anim_script as _anim
from . import scene as _scene
from .anim_script import (DCO_SCRIPTS, HANDLE_SCRIPTS, HOLD_SCRIPTS, INITVEL_SCRIPTS, PULL_SCRIPTS, RULE_SCRIPTS,  # noqa: F401  (the scripts themselves
                          UnsupportedKeyword)  # are restated in anim_script.py; their names stay importable from here)

VIEWER_KEYWORDS = {"view", "zoom", "cameraTracking", "playBackSpeed", "appendStr", "disableCout", "section"}


def _rot(deg):
    """Rx Ry Rz of Euler angles in degrees (Config.cpp:222-226)."""
    x, y, z = (math.radians(a) for a in deg)
    cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


@dataclass
class Shape:
    path: str
    translate: np.ndarray
    rotate_deg: np.ndarray
    scale: np.ndarray
    material: tuple = None  # (rho, E, nu)
    lin_vel: tuple = None  # scripted (kinematic component)
    ang_vel_deg: tuple = None
    init_vel: tuple = None  # (linear, angular deg/s)
    mesh_seq: str = None  # `meshSeq <folder>`: the component follows the positions of <folder>/<step>.{msh,obj,seg,pt} (Config.cpp:284-289)
    dbc: list = field(default_factory=list)  # (rel_min, rel_max, lin_vel, ang_vel_deg, t0, t1)
    nbc: list = field(default_factory=list)  # (rel_min, rel_max, acceleration, t0, t1)
    contact_group: int = 0  # `contactGroup g` (this project's keyword): the contact group of the component, see SceneConfig.contact_group_tables
    # `shell <thickness> [bend <scale>]` (this project's keyword, triangle meshes only): the component is an elastic shell -- membrane and bending energy with
    # the shape's `material` or the scene's density / stiffness (Context.set_shell) -- and may be free, partly held by `DBC` boxes or moved by the scripts
    shell_thickness: float = None
    shell_bend: float = 1.0
    # `shell <thickness> [bend <scale>] [limit <s> [onset <sHat>] [stiff <k>]]`: strain limiting of this shape's triangles -- a barrier on their principal
    # stretches that starts at the onset (default 1) and is infinite at the limit (Context.set_shell_strain_limit); per shape, shapes may differ
    shell_limit: float = None
    shell_onset: float = 1.0
    shell_stiff: float = 1.0
    # `shell <thickness> [bend <scale>] [rubber [mr <alpha>]] [limit ...]`: this shape's triangles carry the incompressible Mooney-Rivlin membrane in place of
    # the StVK one (Context.set_shell_membrane); alpha in [0, 1) is the I2 fraction, default 0 = neo-Hookean; per shape, shapes may differ
    shell_rubber: bool = False
    # `shell <thickness> [bend <scale>] weave <E1> <E2> <G12> dir <x> <y> <z> [nu12 <v>] [bendwarp <s>] [bendweft <s>] [limit ...]`: this shape's triangles are woven
    # cloth -- an orthotropic StVK membrane with Young's moduli E1 along the warp and E2 along the weft, the shear modulus G12 and Poisson's ratio nu12 (default
    # 0), and bending factors about the two yarn directions (default 1 1) -- in place of the isotropic one (Context.set_shell_weave;
    # ipc_amd/csrc/shell_weave_kernels.h).  dir is the warp in the mesh file's frame; it turns (and scales) with the shape line's transform and is projected into
    # every triangle.  Stands where `rubber` does; not with `rubber` or `yield`.  {E1, E2, G12, dir, nu12, bendwarp, bendweft}, or None
    shell_weave: dict = None
    # `shell <thickness> [bend <s>] [limit ...] yield <y> [bendyield <yb>] [creep <rate>] [harden <K>]`: this shape's triangles flow plastically -- the membrane
    # where the deviatoric Hencky strain norm exceeds y + K alpha, a hinge where its outer-fibre strain exceeds yb + K alphaB (Context.shell_set_plasticity);
    # bendyield defaults to yield, creep to inf (returned within the step), harden to 0; not with `rubber`.  (yield, bendyield, creep, harden), or None
    shell_plastic: tuple = None
    # `plastic <yield> [creep <rate>] [harden <K>]` (this project's keyword, tetrahedral shapes only): the shape's elements flow plastically where the deviatoric
    # Hencky strain norm exceeds yield + K alpha (Context.set_plasticity; for small strains the von Mises stress is sqrt(6) mu n); creep: the rate at which the
    # excess decays (default inf: returned within the step), harden: isotropic hardening (default 0).  (yield, creep, harden), or None
    plastic: tuple = None
    # `fiber <k> dir <x> <y> <z> [exp <k2>] [tensiononly] [activate <act> [ramp <seconds>]]` (this project's keyword, tetrahedral shapes only): one fibre family
    # in the shape's elements (Context.set_fibers; ipc_amd/csrc/fiber_kernels.h).  k is a stress; dir is in the mesh file's frame and turns (and scales) with
    # the shape line's transform; `exp <k2>` picks the exponential law (no activation with it), `tensiononly` lets spring fibres buckle; `activate` makes
    # them want the stretch 1 - act, with `ramp` reached linearly over that many seconds (tools/run_scene.py sets act min(1, t / ramp) before each step).
    # {k, dir, law, k2, tension_only, act, ramp}, or None
    fiber: dict = None
    shell_alpha: float = 0.0
    # `rod <radius> [bend <scale>]` (this project's keyword, `.seg` shapes only): the component is an elastic rod -- stretching and bending energy with the
    # shape's `material` or the scene's density / stiffness (Context.set_rod; Poisson's ratio is unused) -- and may be free or partly held by `DBC` boxes
    rod_radius: float = None
    rod_bend: float = 1.0
    # `pressure <p> [ramp <seconds>]` (this project's keyword, on a `shell` shape or a tetrahedral shape): the shape's surface triangles -- the shell's own, or
    # the boundary faces of the tetrahedra -- are ONE pressure chamber with the constant gauge pressure p (positive pushes outward; Context.set_chambers).  The
    # surface must be closed (an open one is a ValueError that names the shape); where its triangle list encloses a negative volume the CHAMBER's copy of the
    # list is flipped, never the shell's own.  With `ramp` the pressure of the step that ends at time t is p min(1, t / ramp) (tools/run_scene.py sets it
    # before each step through AssembledScene.chamber_pressures and Context.chamber_set_pressure).  `gas <ambient> [gamma <g>]` behind them makes it a gas
    # chamber (Context.chamber_set_gas): an ideal gas of the ambient absolute pressure <ambient> >= 0 and the exponent g >= 1 (default 1, isothermal; 1.4 is
    # adiabatic air), filled at the rest volume; p is then the gauge pressure at the rest volume, ambient + p > 0, and a `ramp` pumps the gas in
    pressure: float = None
    pressure_ramp: float = 0.0
    # `aero [cn <C>] [ct <C>] [onesided]` (this project's keyword, on a `shell` shape or a tetrahedral shape): the shape's surface triangles are ONE
    # aerodynamic surface with the normal and tangential drag coefficients cn >= 0 (default 1.28, a flat plate) and ct >= 0 (default 0) in the scene's
    # `wind` (Context.set_aero).  On a `shell` shape the triangles are the shell's own, two-sided unless `onesided` is given; on a tetrahedral shape they are
    # the outward boundary faces, always one-sided (only the face that pushes into the air is loaded)
    aero: bool = False
    aero_cn: float = 1.28
    aero_ct: float = 0.0
    aero_onesided: bool = False
    pressure_gas: bool = False
    pressure_ambient: float = 0.0
    pressure_gamma: float = 1.0


def _parse_round_collider(k, a):
    """sphereCollider cx cy cz R [hollow] [friction mu] [velocity vx vy vz]  /  capsuleCollider ax ay az bx by bz R [friction mu] [velocity vx vy vz]
    -> {p0, p1, R, hollow, friction, velocity (None: at rest)}"""
    sphere = k == "sphereCollider"
    usage = (k + " needs <cx> <cy> <cz> <R> [hollow] [friction <mu>] [velocity <vx> <vy> <vz>]") if sphere else (
        k + " needs <ax> <ay> <az> <bx> <by> <bz> <R> [friction <mu>] [velocity <vx> <vy> <vz>]")
    nNum = 4 if sphere else 7
    try:
        v = [float(x) for x in a[:nNum]]
    except ValueError:
        raise ValueError(usage) from None
    if len(v) < nNum:
        raise ValueError(usage)
    out = {"p0": np.array(v[0:3]), "p1": np.array(v[0:3] if sphere else v[3:6]), "R": v[nNum - 1], "hollow": False, "friction": 0.0, "velocity": None}
    j, seen = nNum, set()
    while j < len(a):
        word = a[j]
        if word in seen:
            raise ValueError(f"{k}: {word} is given twice")
        seen.add(word)
        try:
            if word == "hollow" and sphere:
                out["hollow"] = True
                j += 1
            elif word == "friction" and j + 1 < len(a):
                out["friction"] = float(a[j + 1])
                j += 2
            elif word == "velocity" and j + 3 < len(a):
                out["velocity"] = np.array([float(x) for x in a[j + 1:j + 4]])
                j += 4
            elif word == "hollow":
                raise ValueError(f"{k}: only a sphere may be hollow")
            else:
                raise ValueError(usage)
        except ValueError as e:
            raise ValueError(str(e) if str(e).startswith(k) else usage) from None
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"{k}: the coordinates and the radius must be finite")
    if not out["R"] > 0.0:
        raise ValueError(f"{k}: the radius must be positive")
    if not sphere and np.array_equal(out["p0"], out["p1"]):
        raise ValueError(f"{k}: the two end points coincide (that is a sphereCollider)")
    if not (math.isfinite(out["friction"]) and out["friction"] >= 0.0):
        raise ValueError(f"{k}: the friction coefficient must be finite and not negative")
    if out["velocity"] is not None and not np.all(np.isfinite(out["velocity"])):
        raise ValueError(f"{k}: the velocity must be finite")
    return out


@dataclass
class SceneConfig:
    energy: str = "NH"
    time_integration: str = "BE"
    linear_solver: int = 0  # `linearSolver` (Config.cpp:120-124): the solver type of ipcgpu_ctx_set_solver, for the Context the caller creates
    beta: float = 0.25
    gamma: float = 0.5
    duration: float = 5.0
    dt: float = 0.025
    rho: float = 1000.0
    YM: float = 1e5
    PR: float = 0.4
    gravity: bool = True
    self_collision: bool = True  # Config.hpp:99
    self_fric: float = 0.0
    dHat_eps: float = 1e-3  # tuning[1]
    eps_v: float = 1e-3  # tuning[4]
    eps_v_target: float = -1.0  # tuning[5]; < 0: the same as eps_v (the `epsv` keyword sets both)
    handle_ratio: float = 0.01  # `handleRatio r` (Config.cpp:528-531): the width, in bounding-box extents, of the border slabs the handle scripts take (main.cpp:1180)
    dbc_time_range: tuple = (0.0, math.inf)  # `DBCTimeRange t0 t1` (Config.cpp:175-177): every Dirichlet group acts inside it only (AnimScripter.cpp:99, 1440)
    nbc_time_range: tuple = (0.0, math.inf)  # `NBCTimeRange t0 t1` (Config.cpp:178-180; AnimScripter.cpp:2372-2375)
    dtol_rel: float = 1e-9  # tuning[3] (Optimizer.cpp:102-106)
    use_abs_parameters: bool = False  # Config.cpp:553-555: the lengths of `tuning` and the tolerance are absolute
    kappa_min_multiplier: float = 1e11  # Config.cpp:556-558, Config.hpp:139
    fric_iter_amt: int = 1
    rot_axis: tuple = (0.0, 0.0, 0.0)  # rotateModel ax ay az deg (Config.cpp:523-526)
    rot_deg: float = 0.0
    kappa: float = 0.0  # tuning[0]; 0 = suggestKappa
    dHat_target: float = -1.0  # tuning[2]; < 0: the same as dHat (no homotopy)
    damping_stiff: float = 0.0  # Config.cpp:141-147; `dampingRatio r` becomes r * dt^3 * 3 / 4 once the file is read (:614-616)
    damping_ratio: float = 0.0
    tol: float = 1e-2
    script: str = "null"
    script_params: list = field(default_factory=list)
    script_seq_folder: str = None  # `script meshSeqFromFile <folder>`
    size: float = -1.0  # > 0: the assembled model is scaled so that its largest extent is `size` and moved to the origin (main.cpp:1140-1145)
    warm_start: int = 0  # initX option
    restart: str = None
    half_spaces: list = field(default_factory=list)  # (origin, normal, friction)
    round_colliders = ()  # `sphereCollider` / `capsuleCollider` lines, see _parse_round_collider (a plain attribute, not a field: a scene without them has the fields it had)
    mesh_cos: list = field(default_factory=list)  # (obj path, origin, scale, friction, rotate_deg) -- kinematic mesh obstacles (MeshCO)
    shapes: list = field(default_factory=list)
    # contact groups (this project's keywords, not the reference's): `contactIgnore g h` -- groups g and h form no contact pair --, `contactFric g h mu` -- the
    # friction coefficient between groups g and h --, and a trailing `contactGroup g` on a shape line (Shape.contact_group)
    contact_ignore: list = field(default_factory=list)  # (g, h)
    contact_fric: list = field(default_factory=list)  # (g, h, mu)
    # `attach <shapeA> <nodeA> <shapeB> <nodeB> <k> [<L>]` and `stitch <shapeA> <shapeB> <radius> <k> [rest]` (this project's keywords, top-level lines):
    # springs W = k (|x_A - x_B| - L)^2 / 2 between nodes of two shapes (Context.set_attachments).  Shapes count the `shapes` block from 0, nodes are local
    # to their shape.  `attach` ties one pair (L defaults to 0).  `stitch` ties every node of shape A whose rest position (after the shape's transform) lies
    # within <radius> of a node of shape B to its nearest such node, with L = 0 or, with `rest`, the rest distance of the pair; one that ties nothing is
    # an error.  Contact between the two shapes is not changed: mask it with contactGroup / contactIgnore, or give a rest length.
    attach: list = field(default_factory=list)  # (shapeA, nodeA, shapeB, nodeB, k, L)
    stitch: list = field(default_factory=list)  # (shapeA, shapeB, radius, k, rest)
    # `wind <wx> <wy> <wz> [density <rho>]` (this project's keyword, a top-level line): the wind velocity, uniform in space, and the air density the `aero`
    # shapes see (Context.aero_set_wind).  Default: still air of density 1.225
    wind: tuple = (0.0, 0.0, 0.0)
    air_density: float = 1.225

    def uses_contact_groups(self):
        return bool(self.contact_ignore or self.contact_fric or any(sh.contact_group for sh in self.shapes))

    def effective_self_fric(self):
        """selfFric as the library gets it: the largest coefficient of the scene, the pairs of groups carry ratios to it (contact_group_tables)."""
        return max([self.self_fric] + [mu for _, _, mu in self.contact_fric])

    def contact_group_tables(self, n_components=None):
        """What `contactGroup` / `contactIgnore` / `contactFric` amount to, as Context.set_contact_groups takes it: None for a scene without these
        keywords, else (groups[n_components], collide[n, n], fric_scale[n, n] or None, self_fric).  Components behind the shapes (mesh collision
        objects) are in group 0.  A pair of groups without a `contactFric` line carries the scene's selfFric; self_fric is the largest coefficient and
        fric_scale holds the ratios to it (None: no `contactFric` line, or no friction at all).  A later line for the same pair replaces an earlier one."""
        if not self.uses_contact_groups():
            return None
        n_components = len(self.shapes) if n_components is None else n_components
        if n_components < len(self.shapes):
            raise ValueError("contact groups: fewer components than shapes")
        groups = np.zeros(n_components, dtype=np.int32)
        groups[:len(self.shapes)] = [sh.contact_group for sh in self.shapes]
        n = 1 + max([int(groups.max())] + [max(g, h) for g, h, *_ in self.contact_ignore + self.contact_fric])
        collide = np.ones((n, n), dtype=np.uint8)
        for g, h in self.contact_ignore:
            collide[g, h] = collide[h, g] = 0
        mu_max = self.effective_self_fric()
        fric_scale = None
        if self.contact_fric and mu_max > 0:
            fric_scale = np.full((n, n), self.self_fric / mu_max)
            for g, h, mu in self.contact_fric:
                fric_scale[g, h] = fric_scale[h, g] = mu / mu_max
        return groups, collide, fric_scale, mu_max

    @staticmethod
    def parse(text, base_dir="."):
        cfg = SceneConfig()
        lines = text.splitlines()
        i = 0

        def resolve(p):
            return p if os.path.isabs(p) else os.path.normpath(os.path.join(base_dir, p))

        while i < len(lines):
            tok = lines[i].split()
            i += 1
            if not tok or tok[0].startswith("#"):
                continue
            k, a = tok[0], tok[1:]
            if k == "energy":
                if a[0] not in ("NH", "FCR", "SNH"):  # SNH: stable neo-Hookean, this project's third energy (not a keyword of the reference)
                    raise UnsupportedKeyword(f"energy {a[0]}")
                cfg.energy = a[0]
            elif k == "timeIntegration":
                cfg.time_integration = a[0]
                if a[0] == "NM" and len(a) >= 3:
                    cfg.beta, cfg.gamma = float(a[1]), float(a[2])
                elif a[0] not in ("BE", "NM"):
                    raise UnsupportedKeyword(f"timeIntegration {a[0]}")
            elif k == "time":
                cfg.duration, cfg.dt = float(a[0]), float(a[1])
            elif k == "density":
                cfg.rho = float(a[0])
            elif k == "stiffness":
                cfg.YM, cfg.PR = float(a[0]), float(a[1])
            elif k == "turnOffGravity":
                cfg.gravity = False
            elif k == "script":
                if a[0] not in ("null", "twist", "fall", "fallNoShift", "dragright", "DCOFix", "DCOBallHitWall", "stretchAndPause", "meshSeqFromFile", "ACOSquash", "ACOSquash6", "DCOHammerWalnut", "DCOCut") + HANDLE_SCRIPTS + HOLD_SCRIPTS + PULL_SCRIPTS + INITVEL_SCRIPTS + RULE_SCRIPTS and a[0] not in DCO_SCRIPTS:
                    raise UnsupportedKeyword(f"script {a[0]}")
                cfg.script = a[0]
                if a[0] == "meshSeqFromFile":  # Config.cpp:161-164: the folder of <n>.obj files follows the name
                    cfg.script_seq_folder = resolve(a[1])
                    a = a[:1] + a[2:]
                if len(a) > 1 and int(a[1]) > 0:  # `script name n p1 .. pn` (Config.cpp:166-175): parameters of the script
                    cfg.script_params = [float(x) for x in a[2:2 + int(a[1])]]
            elif k == "warmStart":  # initX option (Optimizer.cpp:925-1110)
                if int(a[0]) not in (0, 1, 2, 3, 4, 5):
                    raise UnsupportedKeyword(f"warmStart {a[0]}")
                cfg.warm_start = int(a[0])
            elif k == "constraintSolver":
                if a[0] not in ("IP", "interiorPoint"):
                    raise UnsupportedKeyword(f"constraintSolver {a[0]}")
            elif k == "timeStepper":
                if a[0] != "Newton":
                    raise UnsupportedKeyword(f"timeStepper {a[0]}")
            elif k == "shape":  # single shape, identity transform (Config.cpp:188-203)
                if a[0] != "input":
                    raise UnsupportedKeyword(f"shape {a[0]}")
                cfg.shapes.append(Shape(resolve(a[1]), np.zeros(3), np.zeros(3), np.ones(3)))
            elif k == "shapes":
                if a[0] != "input":
                    raise UnsupportedKeyword(f"shapes {a[0]}")
                n = int(a[1])
                got = 0
                while got < n:
                    st = lines[i].split()
                    i += 1
                    if not st or st[0].startswith("#"):
                        continue
                    # a `\` token continues the shape on the next line; a `#` token drops the rest of the line up to a
                    # `\` (Config.cpp:290-305)
                    toks = []
                    while True:
                        cont = False
                        for j, t in enumerate(st):
                            if t == "\\":
                                cont = True
                                break
                            if t.startswith("#"):
                                cont = "\\" in st[j + 1:]
                                break
                            toks.append(t)
                        if not cont or i >= len(lines):
                            break
                        st = lines[i].split()
                        i += 1
                    cfg.shapes.append(_parse_shape(toks, resolve))
                    got += 1
            elif k == "shapeMatrix":  # Config.cpp:319-378: one shape replicated on an nx x ny x nz grid
                if a[0] != "input":
                    raise UnsupportedKeyword(f"shapeMatrix {a[0]}")
                cnt = [int(x) for x in a[1:4]]
                pos = [float(x) for x in a[4:7]] + [0.0] * (3 - len(a[4:7]))
                st = lines[i].split()
                i += 1
                step = np.array([float(x) for x in st[1:4]])
                rot, scl = np.array([float(x) for x in st[4:7]]), np.array([float(x) for x in st[7:10]])
                mat = tuple(float(x) for x in st[11:14]) if len(st) > 13 and st[10] == "material" else None
                for xi in range(cnt[0]):
                    for yi in range(cnt[1]):
                        for zi in range(cnt[2]):
                            cfg.shapes.append(Shape(resolve(st[0]), np.array(pos) + step * np.array([xi, yi, zi]), rot, scl, material=mat))
            elif k == "ground":  # friction, height (Config.cpp:425-430)
                cfg.half_spaces.append((np.array([0.0, float(a[1]), 0.0]), np.array([0.0, 1.0, 0.0]), float(a[0])))
            elif k == "halfSpace":  # origin, normal, stiffness (unused), friction (Config.cpp:431-447)
                v = [float(x) for x in a]
                n = np.array(v[3:6])
                cfg.half_spaces.append((np.array(v[0:3]), n / np.linalg.norm(n), v[7] if len(v) > 7 else 0.0))
            elif k == "meshCO":  # path, origin, scale, stiffness (unused), friction [rotate x y z] (Config.cpp:448-474)
                v = [float(x) for x in a[1:7]]
                rot = np.zeros(3)
                if len(a) > 10 and a[7] == "rotate":
                    rot = np.array([float(x) for x in a[8:11]])
                cfg.mesh_cos.append((resolve(a[0]), np.array(v[0:3]), v[3], v[5], rot))
            elif k == "selfCollisionOn":
                cfg.self_collision = True
            elif k == "selfCollisionOff":
                cfg.self_collision = False
            elif k == "selfFric":
                cfg.self_fric = float(a[0])
            elif k == "dHat":  # Config.cpp:542-545: entries 1 and 2 of `tuning`
                cfg.dHat_eps = cfg.dHat_target = float(a[0])
            elif k == "epsv":  # Config.cpp:546-549: entries 4 and 5 of `tuning`
                cfg.eps_v = float(a[0])
                cfg.eps_v_target = -1.0
            elif k == "fricIterAmt":
                cfg.fric_iter_amt = int(a[0])
            elif k == "tol":
                vals = []
                while len(vals) < int(a[0]):
                    vals += [float(x) for x in lines[i].split()]
                    i += 1
                if vals:
                    cfg.tol = vals[0]
            elif k == "tuning":  # Config.cpp:41-45, 533-541: [kappa (0 = automatic), dHat, dHat target, dTol, eps_v, eps_v target]
                vals = []
                while len(vals) < int(a[0]):
                    vals += [float(x) for x in lines[i].split()]
                    i += 1
                # `tuning.resize(amt)` (Config.cpp:533-541) DROPS the entries the line does not give: whatever an earlier `dHat` / `epsv`
                # keyword had set falls back to the Optimizer's defaults (Optimizer.cpp:276-304: 1e-3 each, kappa automatic)
                cfg.kappa = max(vals[0], 0.0) if len(vals) > 0 else 0.0  # the start value of every time step (Optimizer.cpp:1540-1547)
                cfg.dHat_eps = vals[1] if len(vals) > 1 else 1e-3
                cfg.dHat_target = vals[2] if len(vals) > 2 else 1e-3  # Optimizer.cpp:283-289: without a third entry the target is 1e-3 (relative)
                cfg.dtol_rel = vals[3] if len(vals) > 3 else 1e-9
                cfg.eps_v = vals[4] if len(vals) > 4 else 1e-3
                cfg.eps_v_target = vals[5] if len(vals) > 5 else 1e-3  # Optimizer.cpp:296-299: without a sixth entry the target is 1e-3
            elif k == "handleRatio":
                cfg.handle_ratio = float(a[0])
                if not 0 < cfg.handle_ratio < 0.5:
                    raise ValueError("handleRatio must lie in (0, 0.5) (Config.cpp:530)")
            elif k in ("linearSolver", "linSysSolver"):
                # Config.cpp:120-124, 689-706: `amgcl | AMGCL` is the iterative choice (solver type 2 with the library's defaults); `cholmod | CHOLMOD`,
                # `eigen | EIGEN | Eigen` are exact factorisations, and an unknown name falls back to one with a warning (:704-705): the multifrontal solver
                name = a[0] if a else ""
                if name in ("amgcl", "AMGCL"):
                    cfg.linear_solver = 2
                else:
                    cfg.linear_solver = 0
                    if name not in ("cholmod", "CHOLMOD", "eigen", "EIGEN", "Eigen"):
                        warnings.warn(f"unknown linear system solver: {name}; using the default (multifrontal) solver")
            elif k in ("CCDTolerance", "ccdTolerance"):
                pass  # Config.cpp:569-571: read by the TightInclusion back end only (Optimizer.cpp:1149, 1173); the default method takes none
            elif k == "DBCTimeRange":
                cfg.dbc_time_range = (float(a[0]), float(a[1]))
            elif k == "NBCTimeRange":
                cfg.nbc_time_range = (float(a[0]), float(a[1]))
            elif k == "useAbsParameters":  # Config.cpp:553-555
                cfg.use_abs_parameters = True
            elif k in ("kappaMinMultiplier", "minBarrierStiffnessScale"):  # Config.cpp:556-558
                cfg.kappa_min_multiplier = float(a[0])
            elif k == "section":  # Config.cpp:572-605: settings for one constraint solver; other solvers' sections are skipped
                names = ["interiorPoint" if x == "IP" else x for x in a]
                if "end" not in names and "interiorPoint" not in names:
                    while i < len(lines):
                        t2 = lines[i].split()
                        i += 1
                        if len(t2) >= 2 and t2[0] == "section" and t2[1] == "end":
                            break
            elif k in ("CCDMethod", "ccdMethod"):  # Config.cpp:564-568: only the default method is rebuilt here
                if a[0] != "FloatingPointRootFinder":
                    raise UnsupportedKeyword(f"CCDMethod {a[0]}")
            elif k == "restart":
                cfg.restart = resolve(a[0])
            elif k == "size":  # Config.cpp: `size s`; applied to the whole model after the shapes are assembled (main.cpp:1140-1145)
                cfg.size = float(a[0])
            elif k == "rotateModel":  # Config.cpp:523-526
                cfg.rot_axis, cfg.rot_deg = tuple(float(x) for x in a[:3]), float(a[3])
            elif k == "dampingStiff":  # Config.cpp:141-147
                cfg.damping_stiff = max(float(a[0]), 0.0)
            elif k == "dampingRatio":  # Config.cpp:148-157
                cfg.damping_ratio = min(max(float(a[0]), 0.0), 1.0)
            elif k == "contactIgnore":  # this project's keyword: the two groups form no contact pair (g == h: no contact inside the group either)
                if len(a) < 2:
                    raise ValueError("contactIgnore needs two groups")
                cfg.contact_ignore.append((_contact_group(a[0]), _contact_group(a[1])))
            elif k == "contactFric":  # this project's keyword: friction coefficient between two groups
                if len(a) < 3:
                    raise ValueError("contactFric needs two groups and a coefficient")
                mu = float(a[2])
                if not (math.isfinite(mu) and mu >= 0):
                    raise ValueError("contactFric: the coefficient must be finite and not negative")
                cfg.contact_fric.append((_contact_group(a[0]), _contact_group(a[1]), mu))
            elif k == "attach":  # this project's keyword: one node-to-node attachment
                if len(a) not in (5, 6):
                    raise ValueError("attach needs <shapeA> <nodeA> <shapeB> <nodeB> <k> [<L>]")
                kk, L = float(a[4]), float(a[5]) if len(a) == 6 else 0.0
                if not (math.isfinite(kk) and kk > 0 and math.isfinite(L) and L >= 0):
                    raise ValueError("attach: k must be positive and L must not be negative")
                cfg.attach.append((int(a[0]), int(a[1]), int(a[2]), int(a[3]), kk, L))
            elif k == "stitch":  # this project's keyword: the nodes of shape A near shape B, each tied to its nearest node there
                if len(a) not in (4, 5) or (len(a) == 5 and a[4] != "rest"):
                    raise ValueError("stitch needs <shapeA> <shapeB> <radius> <k> [rest]")
                radius, kk = float(a[2]), float(a[3])
                if not (math.isfinite(radius) and radius >= 0 and math.isfinite(kk) and kk > 0):
                    raise ValueError("stitch: the radius must not be negative and k must be positive")
                cfg.stitch.append((int(a[0]), int(a[1]), radius, kk, len(a) == 5))
            elif k == "wind":  # this project's keyword: the wind the `aero` shapes see
                if len(a) not in (3, 5) or (len(a) == 5 and a[3] != "density"):
                    raise ValueError("wind needs <wx> <wy> <wz> [density <rho>]")
                cfg.wind = (float(a[0]), float(a[1]), float(a[2]))
                if len(a) == 5:
                    cfg.air_density = float(a[4])
                if not all(math.isfinite(v) for v in cfg.wind) or not (0.0 < cfg.air_density < math.inf):
                    raise ValueError("wind: the velocity must be finite and the density positive and finite")
            elif k in ("sphereCollider", "capsuleCollider"):  # this project's keywords: analytic round colliders (round_collider_kernels.h)
                if cfg.round_colliders == ():
                    cfg.round_colliders = []
                cfg.round_colliders.append(_parse_round_collider(k, a))
            elif k in VIEWER_KEYWORDS:
                pass  # viewer / logging only
            elif k in ("resolution", "inexactSolve"):
                pass  # tokens Config::loadFromFile itself has no branch for (Config.cpp:97-617): the reference reads past them
            else:
                raise UnsupportedKeyword(k)
        if cfg.damping_ratio > 0:  # Config.cpp:614-616
            cfg.damping_stiff = cfg.damping_ratio * cfg.dt ** 3 * 3 / 4
        return cfg


def _contact_group(tok):
    g = int(tok)
    if not 0 <= g < 16:
        raise ValueError(f"contact group {g}: groups are numbered 0 .. 15")
    return g


def _parse_shape(st, resolve):
    sh = Shape(resolve(st[0]), np.array([float(x) for x in st[1:4]]), np.array([float(x) for x in st[4:7]]), np.array([float(x) for x in st[7:10]]))
    j = 10
    while j < len(st):
        e = st[j]
        j += 1
        if e == "material":
            sh.material = tuple(float(x) for x in st[j:j + 3])
            j += 3
        elif e == "linearVelocity":
            sh.lin_vel = tuple(float(x) for x in st[j:j + 3])
            j += 3
        elif e == "angularVelocity":
            sh.ang_vel_deg = tuple(float(x) for x in st[j:j + 3])
            j += 3
        elif e == "meshSeq":
            sh.mesh_seq = resolve(st[j])
            j += 1
        elif e == "contactGroup":
            if j >= len(st):
                raise ValueError("contactGroup needs a group")
            sh.contact_group = _contact_group(st[j])
            j += 1
        elif e == "plastic":
            if j >= len(st):
                raise ValueError("plastic needs a yield strain")
            par = {"yield": float(st[j]), "creep": math.inf, "harden": 0.0}
            j += 1
            while j < len(st) and st[j] in ("creep", "harden"):
                if j + 1 >= len(st):
                    raise ValueError(st[j] + " needs a number")
                par[st[j]] = float(st[j + 1])
                j += 2
            if not (par["yield"] >= 0.0 and par["creep"] > 0.0 and 0.0 <= par["harden"] < math.inf):
                raise ValueError("plastic needs a yield strain >= 0, a creep rate > 0 and a finite hardening modulus >= 0")
            sh.plastic = (par["yield"], par["creep"], par["harden"])
        elif e == "fiber":
            if j + 4 >= len(st) or st[j + 1] != "dir":
                raise ValueError("fiber needs <k> dir <x> <y> <z>")
            fb = {"k": float(st[j]), "dir": tuple(float(x) for x in st[j + 2:j + 5]), "law": "spring", "k2": 0.0, "tension_only": False, "act": 0.0, "ramp": 0.0}
            j += 5
            while j < len(st) and st[j] in ("exp", "tensiononly", "activate"):
                if st[j] == "tensiononly":
                    fb["tension_only"] = True
                    j += 1
                    continue
                if j + 1 >= len(st):
                    raise ValueError(st[j] + " needs a number")
                if st[j] == "exp":
                    fb["law"], fb["k2"] = "exp", float(st[j + 1])
                    j += 2
                else:
                    fb["act"] = float(st[j + 1])
                    j += 2
                    if j < len(st) and st[j] == "ramp":
                        if j + 1 >= len(st):
                            raise ValueError("ramp needs a time")
                        fb["ramp"] = float(st[j + 1])
                        j += 2
                        if not (0.0 < fb["ramp"] < math.inf):
                            raise ValueError("ramp needs a positive, finite time")
            if not (0.0 < fb["k"] < math.inf):
                raise ValueError("fiber needs a positive, finite stiffness")
            if not all(math.isfinite(x) for x in fb["dir"]) or not any(x != 0.0 for x in fb["dir"]):
                raise ValueError("fiber needs a finite direction that is not zero")
            if fb["law"] == "exp" and not (0.0 < fb["k2"] < math.inf):
                raise ValueError("exp needs a positive, finite k2")
            if not (math.isfinite(fb["act"]) and fb["act"] < 1.0):
                raise ValueError("activate needs an activation below 1")
            if fb["law"] == "exp" and fb["act"] != 0.0:
                raise ValueError("activate is not defined for exp fibres")
            sh.fiber = fb
        elif e == "shell":
            if j >= len(st):
                raise ValueError("shell needs a thickness")
            sh.shell_thickness = float(st[j])
            j += 1
            if j < len(st) and st[j] == "bend":
                if j + 1 >= len(st):
                    raise ValueError("bend needs a scale")
                sh.shell_bend = float(st[j + 1])
                j += 2
            if not sh.shell_thickness > 0.0 or not sh.shell_bend >= 0.0:
                raise ValueError("shell needs a positive thickness and a bend scale >= 0")
            if j < len(st) and st[j] == "rubber":
                sh.shell_rubber = True
                j += 1
                if j < len(st) and st[j] == "mr":
                    if j + 1 >= len(st):
                        raise ValueError("mr needs a fraction")
                    sh.shell_alpha = float(st[j + 1])
                    j += 2
                if not (np.isfinite(sh.shell_alpha) and 0.0 <= sh.shell_alpha < 1.0):
                    raise ValueError("mr needs a fraction 0 <= alpha < 1")
                if j < len(st) and st[j] in ("bend", "rubber", "mr"):
                    raise ValueError(st[j] + " is misplaced: shell <thickness> [bend <scale>] [rubber [mr <alpha>]] [limit ...]")
            elif j < len(st) and st[j] == "mr":
                raise ValueError("mr belongs behind rubber")
            if j < len(st) and st[j] == "weave":
                if sh.shell_rubber:
                    raise ValueError("weave is not valid behind rubber: a triangle carries one membrane law, the rubber one or the woven one")
                if j + 7 >= len(st) or st[j + 4] != "dir":
                    raise ValueError("weave needs <E1> <E2> <G12> dir <x> <y> <z>")
                wv = {"E1": float(st[j + 1]), "E2": float(st[j + 2]), "G12": float(st[j + 3]), "dir": tuple(float(x) for x in st[j + 5:j + 8]),
                      "nu12": 0.0, "bendwarp": 1.0, "bendweft": 1.0}
                j += 8
                for word in ("nu12", "bendwarp", "bendweft"):
                    if j < len(st) and st[j] == word:
                        if j + 1 >= len(st):
                            raise ValueError(word + " needs a number")
                        wv[word] = float(st[j + 1])
                        j += 2
                if not all(0.0 < wv[k] < math.inf for k in ("E1", "E2", "G12")):
                    raise ValueError("weave needs positive, finite moduli E1, E2 and G12")
                if not all(math.isfinite(x) for x in wv["dir"]) or not any(x != 0.0 for x in wv["dir"]):
                    raise ValueError("weave needs a finite direction that is not zero")
                if not (math.isfinite(wv["nu12"]) and wv["nu12"] ** 2 < wv["E1"] / wv["E2"]):
                    raise ValueError("nu12 needs nu12^2 < E1 / E2: the law is not positive definite otherwise")
                if not all(0.0 < wv[k] < math.inf for k in ("bendwarp", "bendweft")):
                    raise ValueError("bendwarp and bendweft need positive, finite factors")
                sh.shell_weave = wv
                if j < len(st) and st[j] in ("bend", "weave", "dir", "nu12", "bendwarp", "bendweft", "mr"):
                    raise ValueError(st[j] + " is misplaced: shell <thickness> [bend <scale>] weave <E1> <E2> <G12> dir <x> <y> <z> [nu12 <v>] [bendwarp <s>] [bendweft <s>] [limit ...]")
                if j < len(st) and st[j] == "rubber":
                    raise ValueError("rubber is not valid behind weave: a triangle carries one membrane law, the woven one or the rubber one")
            elif j < len(st) and st[j] in ("dir", "nu12", "bendwarp", "bendweft"):
                raise ValueError(st[j] + " belongs behind weave")
            if j < len(st) and st[j] == "limit":
                if j + 1 >= len(st):
                    raise ValueError("limit needs a stretch")
                sh.shell_limit = float(st[j + 1])
                j += 2
                for word, attr in (("onset", "shell_onset"), ("stiff", "shell_stiff")):
                    if j < len(st) and st[j] == word:
                        if j + 1 >= len(st):
                            raise ValueError(word + " needs a value")
                        setattr(sh, attr, float(st[j + 1]))
                        j += 2
                if not (np.isfinite(sh.shell_limit) and sh.shell_onset >= 1.0 and sh.shell_limit > sh.shell_onset and 0.0 < sh.shell_stiff < float("inf")):
                    raise ValueError("limit needs 1 <= onset < limit and a stiffness > 0")
            elif j < len(st) and st[j] in ("onset", "stiff"):
                raise ValueError(st[j] + " belongs behind limit")
            if j < len(st) and st[j] == "yield":
                if sh.shell_rubber:
                    raise ValueError("yield is not valid behind rubber: a rubber membrane has no plastic flow")
                if sh.shell_weave is not None:
                    raise ValueError("yield is not valid behind weave: plastic flow rewrites the rest metric, in which warp and weft would stop being orthonormal")
                if j + 1 >= len(st):
                    raise ValueError("yield needs a strain")
                par = {"yield": float(st[j + 1]), "bendyield": None, "creep": math.inf, "harden": 0.0}
                j += 2
                for word in ("bendyield", "creep", "harden"):
                    if j < len(st) and st[j] == word:
                        if j + 1 >= len(st):
                            raise ValueError(word + " needs a number")
                        par[word] = float(st[j + 1])
                        j += 2
                if par["bendyield"] is None:
                    par["bendyield"] = par["yield"]
                if not (par["yield"] >= 0.0 and par["bendyield"] >= 0.0 and par["creep"] > 0.0 and 0.0 <= par["harden"] < math.inf):
                    raise ValueError("yield needs strains >= 0, a creep rate > 0 and a finite hardening modulus >= 0")
                sh.shell_plastic = (par["yield"], par["bendyield"], par["creep"], par["harden"])
                if j < len(st) and st[j] in ("yield", "bendyield", "creep", "harden", "limit", "onset", "stiff"):
                    raise ValueError(st[j] + " is misplaced: shell <thickness> [bend <s>] [limit ...] yield <y> [bendyield <yb>] [creep <rate>] [harden <K>]")
            elif j < len(st) and st[j] in ("bendyield", "creep", "harden"):
                raise ValueError(st[j] + " belongs behind yield")
            if j < len(st) and st[j] == "weave":
                raise ValueError("weave is misplaced: shell <thickness> [bend <scale>] weave <E1> <E2> <G12> dir <x> <y> <z> [nu12 <v>] [bendwarp <s>] [bendweft <s>] [limit ...]")
            if j < len(st) and st[j] in ("rubber", "mr", "bend"):
                raise ValueError(st[j] + " is misplaced: shell <thickness> [bend <scale>] [rubber [mr <alpha>]] [limit ...]")
        elif e == "rod":
            if j >= len(st):
                raise ValueError("rod needs a radius")
            sh.rod_radius = float(st[j])
            j += 1
            if j < len(st) and st[j] == "bend":
                if j + 1 >= len(st):
                    raise ValueError("bend needs a scale")
                sh.rod_bend = float(st[j + 1])
                j += 2
            if not sh.rod_radius > 0.0 or not sh.rod_bend >= 0.0:
                raise ValueError("rod needs a positive radius and a bend scale >= 0")
        elif e == "pressure":
            if j >= len(st):
                raise ValueError("pressure needs a value")
            sh.pressure = float(st[j])
            j += 1
            if j < len(st) and st[j] == "ramp":
                if j + 1 >= len(st):
                    raise ValueError("ramp needs a time")
                sh.pressure_ramp = float(st[j + 1])
                j += 2
                if not (0.0 < sh.pressure_ramp < float("inf")):
                    raise ValueError("ramp needs a positive, finite time")
            if not np.isfinite(sh.pressure):
                raise ValueError("pressure needs a finite value")
            if j < len(st) and st[j] == "gas":
                if j + 1 >= len(st):
                    raise ValueError("gas needs an ambient pressure")
                sh.pressure_gas = True
                sh.pressure_ambient = float(st[j + 1])
                j += 2
                if j < len(st) and st[j] == "gamma":
                    if j + 1 >= len(st):
                        raise ValueError("gamma needs a value")
                    sh.pressure_gamma = float(st[j + 1])
                    j += 2
                if not (0.0 <= sh.pressure_ambient < float("inf")):
                    raise ValueError("gas needs a finite ambient pressure >= 0")
                if not (1.0 <= sh.pressure_gamma < float("inf")):
                    raise ValueError("gamma needs a finite value >= 1")
                # (with a ramp the pressure starts near 0: the ambient pressure alone must then carry the gas)
                if not sh.pressure_ambient + min(sh.pressure, 0.0 if sh.pressure_ramp > 0.0 else sh.pressure) > 0.0:
                    raise ValueError("gas needs ambient + pressure > 0 (the absolute pressure at the rest volume)")
        elif e == "aero":
            sh.aero = True
            while j < len(st) and st[j] in ("cn", "ct", "onesided"):
                if st[j] == "onesided":
                    sh.aero_onesided = True
                    j += 1
                    continue
                if j + 1 >= len(st):
                    raise ValueError(f"{st[j]} needs a coefficient")
                setattr(sh, "aero_" + st[j], float(st[j + 1]))
                j += 2
            if not (0.0 <= sh.aero_cn < float("inf")) or not (0.0 <= sh.aero_ct < float("inf")):
                raise ValueError("aero needs finite coefficients cn >= 0 and ct >= 0")
        elif e in ("cn", "ct", "onesided"):
            raise ValueError(f"{e} is valid behind aero only")
        elif e == "initVel":
            v = [float(x) for x in st[j:j + 6]]
            sh.init_vel = (tuple(v[:3]), tuple(v[3:]))
            j += 6
        elif e == "DBC":
            v = [float(x) for x in st[j:j + 12]]
            j += 12
            t0, t1 = 0.0, float("inf")
            try:  # optional start / stop time (Config.cpp:251-254)
                t0 = float(st[j])
                j += 1
                t1 = float(st[j])
                j += 1
            except (IndexError, ValueError):
                pass
            sh.dbc.append((v[0:3], v[3:6], v[6:9], v[9:12], t0, t1))
        elif e == "NBC":
            v = [float(x) for x in st[j:j + 9]]
            j += 9
            t0, t1 = 0.0, float("inf")
            try:  # optional start / stop time (Config.cpp:269-272)
                t0 = float(st[j])
                j += 1
                t1 = float(st[j])
                j += 1
            except (IndexError, ValueError):
                pass
            sh.nbc.append((v[0:3], v[3:6], v[6:9], t0, t1))
        else:
            raise UnsupportedKeyword(f"shape keyword {e}")
    if sh.shell_thickness is not None and os.path.splitext(sh.path.lower())[1] != ".obj":
        raise ValueError("shell is valid on a triangle-mesh shape only (not on a tetrahedral, segment or point shape)")
    if sh.rod_radius is not None and os.path.splitext(sh.path.lower())[1] != ".seg":
        raise ValueError("rod is valid on a segment shape only (not on a tetrahedral, triangle-mesh or point shape)")
    if sh.plastic is not None and os.path.splitext(sh.path.lower())[1] in (".obj", ".seg", ".pt"):
        raise ValueError("plastic is valid on a tetrahedral shape only (not on a shell, rod, point or surface-only shape)")
    if sh.fiber is not None and os.path.splitext(sh.path.lower())[1] in (".obj", ".seg", ".pt"):
        raise ValueError("fiber is valid on a tetrahedral shape only (not on a shell, rod, point or surface-only shape)")
    if sh.fiber is not None and sh.plastic is not None:
        raise ValueError("fiber and plastic exclude each other on a shape (the rest shape would flow under the fibre direction)")
    if sh.aero:
        ext = os.path.splitext(sh.path.lower())[1]
        if ext in (".seg", ".pt") or (ext == ".obj" and sh.shell_thickness is None):
            raise ValueError("aero is valid on a shell shape or a tetrahedral shape only (not on a segment, point or kinematic triangle-mesh shape)")
        if ext != ".obj":
            sh.aero_onesided = True  # the boundary faces of a solid have one side in the air
    if sh.pressure is not None:
        ext = os.path.splitext(sh.path.lower())[1]
        if ext in (".seg", ".pt") or (ext == ".obj" and sh.shell_thickness is None):
            raise ValueError("pressure is valid on a shell shape or a tetrahedral shape only (not on a segment, point or kinematic triangle-mesh shape)")
    return sh


def read_obj(path):
    """Triangle mesh of a Wavefront .obj (igl::readOBJ as MeshCO uses it, MeshCO.cpp:49): `v x y z` and `f a b c` lines, 1-based
    indices, `a/b/c` index groups reduced to the vertex index, negative (relative) indices, polygons fan-triangulated."""
    V, F = [], []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                V.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                idx = []
                for g in t[1:]:
                    k = int(g.split("/")[0])
                    idx.append(k - 1 if k > 0 else len(V) + k)
                for q in range(1, len(idx) - 1):
                    F.append([idx[0], idx[q], idx[q + 1]])
    return np.array(V, dtype=np.float64).reshape(-1, 3), np.array(F, dtype=np.int32).reshape(-1, 3)


def read_seg(path):
    """Segment mesh of a `.seg` shape (main.cpp:957-990): IglUtils::readSEG (`v x y z` / `s a b`, 1-based; IglUtils.cpp:146-175) or, when that
    file does not exist, the edges of the triangles of the `.obj` beside it -- each undirected edge once, with the direction it is first
    seen in, in the order of a std::set of pairs."""
    if os.path.exists(path):
        V, E = [], []
        with open(path) as f:
            for line in f:
                t = line.split()
                if not t:
                    continue
                if t[0] == "v":
                    V.append([float(x) for x in t[1:4]])
                elif t[0] == "s":
                    E.append([int(t[1]) - 1, int(t[2]) - 1])
        return np.array(V, dtype=np.float64).reshape(-1, 3), np.array(E, dtype=np.int32).reshape(-1, 2)
    V, F = read_obj(os.path.splitext(path)[0] + ".obj")
    es = set()
    for a, b, c in F.tolist():
        for i, j in ((a, b), (b, c), (c, a)):
            if (j, i) not in es:
                es.add((i, j))
    return V, np.array(sorted(es), dtype=np.int32).reshape(-1, 2)


def read_pt(path):
    """Point cloud of a `.pt` shape (main.cpp:991-1005): the vertices of the file read as an .obj, or of the `.obj` beside it"""
    if os.path.exists(path):
        return read_obj(path)[0]
    return read_obj(os.path.splitext(path)[0] + ".obj")[0]


def read_seq_file(folder, index, ext):
    """positions of file `index` of a mesh sequence, by the kind of the component that follows it (AnimScripter.cpp:1468-1518)"""
    base = os.path.join(folder, str(index))
    if ext == ".obj":
        return read_obj(base + ".obj")[0]
    if ext == ".seg":
        return read_seg(base + ".seg")[0]
    return read_pt(base + ".pt")


@dataclass
class AssembledScene:
    cfg: SceneConfig
    V: np.ndarray
    T: np.ndarray
    SF: np.ndarray
    node_ranges: list
    tet_ranges: list
    dirichlet: list  # (ids, lin_vel, ang_vel_deg, t0, t1)
    velocity: np.ndarray
    neumann: list = field(default_factory=list)  # (ids, acceleration, t0, t1)
    obstacle_nodes: np.ndarray = None  # nodes of the kinematic mesh obstacles (surface-only components, no tetrahedra)
    release: dict = None  # state-dependent end of a scripted handle (`script dragright`)
    codim_nodes: np.ndarray = None  # surface-only nodes of the mesh itself (triangle meshes under `shapes`, componentCoDim 2) ...
    codim_mass: np.ndarray = None  # ... and their lumped masses (density x a third of the adjacent triangle areas, Mesh.cpp:310-345)
    codim_fixed: np.ndarray = None  # `script DCOFix`: those of them held as NONZERO Dirichlet nodes (AnimScripter.cpp:1222-1236)
    V0: np.ndarray = None  # start positions when they differ from the rest shape V (`rotateModel`, main.cpp:1115-1139)
    codim_edges: np.ndarray = None  # segments of the `.seg` shapes (Mesh::CE), global node pairs
    mesh_seqs: list = None  # `meshSeq` components: {ids, folder, ext, group}
    mesh_i: int = 0  # AnimScripter::meshI: index of the next file of the sequences
    read_seq: object = None  # (folder, index, ext) -> positions; None = the files themselves (tests hand in a fixture's)
    motions: list = None  # rule-driven scripts: per Dirichlet group (lin, ang in degrees, fixed rotation centre or None), nodes NONZERO throughout
    # the shapes that carry `shell`, as Context.set_shell takes them: {tri, thickness, YM, PR, rho (per triangle), bend (one scale for the scene)}, or None;
    # with `limit` on a shape also {limit, onset, stiff (per triangle; limit 0 on the triangles of a shape without it)} for Context.set_shell_strain_limit
    shell: dict = None
    # the shapes that carry `rod`, as Context.set_rod takes them: {seg, radius, YM, rho (per segment), bend (one scale for the scene)}, or None
    rod: dict = None
    # every `attach` and `stitch` line, as Context.set_attachments takes them: {nodesA, nodesB (global node ids), k, L (per attachment)}, or None
    attachments: dict = None
    # the shapes that carry `pressure`, one chamber each in script order, as Context.set_chambers takes them: {tri_lists (global node ids, outward),
    # pressure, ramp (seconds per chamber, 0: none)}, or None.  Where a shape carries `gas` the dictionary also holds gas (bool), ambient and gamma per chamber,
    # as Context.chamber_set_gas takes them
    chambers: dict = None
    # the shapes that carry `aero`, one aerodynamic surface each in script order, as Context.set_aero takes them: {tri_lists (global node ids), cn, ct,
    # one_sided (per surface)}, or None.  Set by assemble(); a plain attribute, not a field, so that the fields of a scene without the keyword are what
    # they were.  The wind itself is the scene's (cfg.wind, cfg.air_density)
    aero = None
    # the shapes that carry `fiber`, in script order, as Context.set_fibers takes them: a list of {tet_range, dir (turned and scaled with the shape), k, law,
    # k2, tension_only, group (the index in this list), act, ramp}, or None.  A plain attribute like `aero`
    fibers = None

    def fiber_activations(self, t):
        """(group, activation) of every `fiber ... activate <act> ramp <seconds>` shape for the time step that ends at time t: act min(1, t / ramp); None when
        no shape has a ramp (then the activations set by apply() stay)"""
        q = [f for f in (self.fibers or []) if f["ramp"] > 0.0]
        if not q:
            return None
        return [(f["group"], f["act"] * min(1.0, t / f["ramp"])) for f in q]

    def move_round_colliders(self, be):
        """Before a time step: every `sphereCollider` / `capsuleCollider` with a `velocity` moves by v dt through Context.round_move; the fraction a
        move leaves over is carried into the next step's, as the half-space scripts do.  Returns the fractions left (one per moving collider)."""
        if not hasattr(self, "_round_carry"):
            self._round_carry = {}
        left = []
        for idx, rc in enumerate(self.cfg.round_colliders):
            if rc["velocity"] is None:
                continue
            delta = np.asarray(rc["velocity"], dtype=np.float64) * self.cfg.dt + self._round_carry.get(idx, 0.0)
            f = be.round_move(idx, delta, 0.5)
            self._round_carry[idx] = f * delta
            left.append(f)
        return left

    def chamber_pressures(self, t):
        """the pressures of the chambers for the time step that ends at time t: p min(1, t / ramp) where a shape gives `ramp`, p elsewhere; None when no
        shape has a ramp (then the pressures set by apply() stay)"""
        q = self.chambers
        if q is None or not np.any(q["ramp"] > 0.0):
            return None
        with np.errstate(divide="ignore"):
            return q["pressure"] * np.where(q["ramp"] > 0.0, np.minimum(1.0, t / np.where(q["ramp"] > 0.0, q["ramp"], 1.0)), 1.0)

    def before_step(self, be, t):
        """What AnimScripter::stepAnimScript decides from the state before a time step (call with the step's start time)."""
        if self.mesh_seqs:
            # AnimScripter.cpp:1465-1532: <folder>/<meshI>.{obj,seg,pt} read as main.cpp reads the shape itself (file positions as they are,
            # NOT moved by the shape's translation / rotation / scale); meshI counts the time steps
            for q in self.mesh_seqs:
                be.set_dirichlet_targets(q["group"], (self.read_seq or read_seq_file)(q["folder"], self.mesh_i, q["ext"]))
            self.mesh_i += 1
        r = self.release
        if r is None or r["done"]:
            return False
        x = np.asarray(be.state()["V"]).reshape(-1, 3)
        return _anim.RULES[r.get("kind", "dragright")](self, r, be, x, t)  # (the dictionary of `dragright` carries no `kind`)


def _attachments(cfg, Vs, nr):
    """the `attach` and `stitch` lines over the transformed shapes Vs (node offsets nr) -> {nodesA, nodesB, k, L} in script order (attach lines first), or None"""
    def shape(s, line):
        if not 0 <= s < len(Vs):
            raise ValueError(f"{line}: shape {s} does not exist (the scene has {len(Vs)})")
        return s
    A, B, K, L, R = [], [], [], [], []  # (R: L is the rest distance of the pair, taken from the assembled rest shape)
    for sa, na, sb, nb_, k, l0 in cfg.attach:
        for s, n in ((shape(sa, "attach"), na), (shape(sb, "attach"), nb_)):
            if not 0 <= n < len(Vs[s]):
                raise ValueError(f"attach: node {n} does not exist in shape {s} ({len(Vs[s])} nodes)")
        if (sa, na) == (sb, nb_):
            raise ValueError(f"attach: node {na} of shape {sa} is tied to itself")
        A.append(nr[sa] + na)
        B.append(nr[sb] + nb_)
        K.append(k)
        L.append(l0)
        R.append(False)
    for sa, sb, radius, k, rest in cfg.stitch:
        if shape(sa, "stitch") == shape(sb, "stitch"):
            raise ValueError("stitch: the two shapes must differ")
        d = np.linalg.norm(Vs[sa][:, None, :] - Vs[sb][None, :, :], axis=2)
        near = d.argmin(axis=1)
        dist = d[np.arange(len(near)), near]
        tied = np.flatnonzero(dist <= radius)
        if not len(tied):
            raise ValueError(f"stitch {sa} {sb}: no node of shape {sa} lies within {radius:g} of a node of shape {sb} (the nearest pair is {dist.min():g} apart)")
        A += (nr[sa] + tied).tolist()
        B += (nr[sb] + near[tied]).tolist()
        K += [k] * len(tied)
        L += [0.0] * len(tied)
        R += [bool(rest)] * len(tied)
    if not A:
        return None
    return {"nodesA": np.array(A, dtype=np.int32), "nodesB": np.array(B, dtype=np.int32), "k": np.array(K, dtype=np.float64), "L": np.array(L, dtype=np.float64),
            "rest": np.array(R, dtype=bool)}


def _chamber_list(SF, V, name):
    """the chamber of one shape: its surface triangles SF (node ids into V) as a closed, outward-oriented list.  ValueError naming the shape where an edge is
    not shared by exactly two triangles that walk it in opposite directions; a list that encloses a negative volume is returned flipped (a copy)."""
    tri = np.array(SF, dtype=np.int32).reshape(-1, 3)
    if len(tri) == 0:
        raise ValueError(f"pressure: {name} has no surface triangle")
    uses = {}
    for t in tri:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            uses.setdefault((min(int(a), int(b)), max(int(a), int(b))), []).append(a < b)
    for (a, b), d in uses.items():
        if len(d) != 2:
            raise ValueError(f"pressure: the surface of {name} is open or not a manifold (edge {a} - {b} belongs to {len(d)} of its triangles, not to two)")
        if d[0] == d[1]:
            raise ValueError(f"pressure: the surface of {name} is not consistently oriented (two triangles walk edge {a} - {b} in the same direction)")
    y = V[tri] - V[np.unique(tri)].mean(axis=0)
    if np.einsum("ti,ti->", y[:, 0], np.cross(y[:, 1], y[:, 2])) < 0.0:
        tri = np.ascontiguousarray(tri[:, ::-1])
    return tri


@dataclass
class _Parts:
    """what the loop over the shapes collects: the transformed meshes with global indices, and what the shapes' own keywords ask for"""
    Vs: list = field(default_factory=list)
    Ts: list = field(default_factory=list)
    SFs: list = field(default_factory=list)
    CEs: list = field(default_factory=list)
    nr: list = field(default_factory=lambda: [0])  # node ranges
    tr: list = field(default_factory=lambda: [0])  # tetrahedron ranges
    codim: list = field(default_factory=list)  # (node ids, triangles, moved by its own keywords, segments) of the components of the mesh without tetrahedra
    given: _anim.ScriptSetup = field(default_factory=_anim.ScriptSetup)  # the Dirichlet / Neumann sets and mesh sequences of the shapes' keywords
    shells: list = field(default_factory=list)  # (triangles, thickness, bend scale, (rho, E, nu), (limit or 0, onset, stiffness), (model, alpha)) per `shell` shape
    rods: list = field(default_factory=list)  # (segments, radius, bend scale, (rho, E, nu)) per `rod` shape
    chambers: list = field(default_factory=list)  # (triangle list, pressure, ramp, (gas, ambient, gamma)) per `pressure` shape
    aero: list = field(default_factory=list)  # (triangle list, cn, ct, one-sided) per `aero` shape


def _read_shape(sh, read_mesh):
    """(ext, V, T, SF, E) of a shape as its file gives it.  main.cpp:948-1005: `.obj` / `.seg` / `.pt` are kinematic surface / segments / points
    (componentCoDim 2 / 1 / 0), components without tetrahedra"""
    ext = os.path.splitext(sh.path.lower())[1]
    T, SF, E = np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2), dtype=np.int32)
    if ext == ".obj":
        V, SF = read_obj(sh.path)
    elif ext == ".seg":
        V, E = read_seg(sh.path)
    elif ext == ".pt":
        V = read_pt(sh.path)
    else:
        V, T, SF = read_mesh(sh.path)
    return ext, V, T, SF, E


def _outward_faces(SF, T, V):
    """the boundary faces SF of the tetrahedra T (node ids into V), each turned so that its normal (right-hand rule) points away from the fourth node of its
    tetrahedron: outward, piece by piece, on the transformed shape (a mirroring scale flips the file's orientation)"""
    apex = {}
    for t in np.asarray(T):
        for k in range(4):
            apex[tuple(sorted(int(v) for v in np.delete(t, k)))] = int(t[k])
    tri = np.array(SF, dtype=np.int32).reshape(-1, 3)
    for i, f in enumerate(tri):
        a = apex.get(tuple(sorted(int(v) for v in f)))
        if a is None:
            raise ValueError(f"aero: surface triangle {i} is no face of a tetrahedron")
        if np.dot(np.cross(V[f[1]] - V[f[0]], V[f[2]] - V[f[0]]), V[a] - V[f[0]]) > 0.0:
            tri[i] = f[::-1]
    return tri


def _weave_record(sh):
    """the `weave` part of a shell shape with the warp turned and scaled like the shape (as a fibre direction is: _fiber_payload), or None"""
    if sh.shell_weave is None:
        return None
    d = _rot(sh.rotate_deg) @ (np.asarray(sh.shell_weave["dir"], dtype=np.float64) * sh.scale)
    return dict(sh.shell_weave, dir=d / np.linalg.norm(d))


def _codim_keywords(cfg, sh, name, V, T, SF, E, off, p):
    """the `shell`, `rod`, `pressure` and `aero` keywords of one shape (transformed nodes V, first node `off`) as records of p"""
    mat = sh.material if sh.material is not None and all(np.isfinite(sh.material)) else (cfg.rho, cfg.YM, cfg.PR)
    if sh.shell_thickness is not None:  # (a triangle mesh: _parse_shape refuses the keyword on any other shape)
        p.shells.append((SF + off, sh.shell_thickness, sh.shell_bend, mat, (0.0, 1.0, 1.0) if sh.shell_limit is None else (sh.shell_limit, sh.shell_onset, sh.shell_stiff),
                         (1, sh.shell_alpha) if sh.shell_rubber else (0, 0.0), sh.shell_plastic, _weave_record(sh)))
    if sh.rod_radius is not None:  # (a segment mesh: _parse_shape refuses the keyword on any other shape)
        p.rods.append((E + off, sh.rod_radius, sh.rod_bend, mat))
    if sh.pressure is not None:  # (a shell or a tetrahedral shape: _parse_shape refuses the keyword on any other); on the transformed shape: a mirroring scale flips it
        p.chambers.append((_chamber_list(SF, V, name) + off, sh.pressure, sh.pressure_ramp, (sh.pressure_gas, sh.pressure_ambient, sh.pressure_gamma)))
    if sh.aero:  # (a shell or a tetrahedral shape: _parse_shape refuses the keyword on any other): the shell's own triangles as they are, or the outward boundary faces
        if len(SF) == 0:
            raise ValueError(f"aero: {name} has no surface triangle")
        tri = np.array(SF, dtype=np.int32).reshape(-1, 3) if sh.shell_thickness is not None else _outward_faces(SF, T, V)
        p.aero.append((tri + off, sh.aero_cn, sh.aero_ct, sh.aero_onesided))


def _assemble_shapes(cfg, read_mesh):
    """main.cpp:880-1077: select Dirichlet / Neumann nodes per shape on the mesh as read, transform the shape (R (p * scale) + translate), concatenate."""
    p = _Parts()
    for s_index, sh in enumerate(cfg.shapes):
        ext, V, T, SF, E = _read_shape(sh, read_mesh)
        is_codim = ext in (".obj", ".seg", ".pt")
        off = p.nr[-1]
        # Dirichlet / Neumann nodes are picked on the mesh AS READ (IglUtils::Init_Dirichlet on newV, main.cpp:1045-1068); the
        # shape is scaled / rotated / translated only afterwards (main.cpp:1073-1077), so the relative box follows the shape
        # (the reference picks among the nodes of surface triangles; a `rod` shape has none: its boxes pick among the nodes of its segments)
        pick = E if sh.rod_radius is not None else SF
        for rel_min, rel_max, lin, ang, t0, t1 in sh.dbc:
            ids = _scene.select_dirichlet(V, pick, rel_min, rel_max)
            if len(ids):
                p.given.dirichlet.append((ids + off, lin, ang, t0, t1))
        for rel_min, rel_max, acc, t0, t1 in sh.nbc:  # same vertex selection (main.cpp:1057-1068)
            ids = _scene.select_dirichlet(V, pick, rel_min, rel_max)
            if len(ids):
                p.given.neumann.append((ids + off, acc, t0, t1))
        V = (V * sh.scale) @ _rot(sh.rotate_deg).T + sh.translate
        if sh.lin_vel is not None or sh.ang_vel_deg is not None:  # scripted component: every node moves (AnimScripter.cpp:1413-1435)
            ids = np.arange(V.shape[0], dtype=np.int32) + off
            p.given.dirichlet.append((ids, sh.lin_vel or (0, 0, 0), sh.ang_vel_deg or (0, 0, 0), 0.0, float("inf")))
        if sh.mesh_seq is not None:
            # AnimScripter.cpp:1465-1528: every node of the component is moved to the positions of the next file of the sequence before each
            # step.  The nodes carry the type their velocities give them: a codimensional component without velocities is held (ZERO, :62-70)
            if cfg.script != "null":
                raise UnsupportedKeyword("meshSeq under a script other than null")
            if not is_codim:
                raise UnsupportedKeyword("meshSeq on a tetrahedral component (its nodes are free: the sequence would only nudge them)")
            ids = np.arange(V.shape[0], dtype=np.int32) + off
            p.given.dirichlet.append((ids, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, float("inf")))
            p.given.seqs.append({"ids": ids, "folder": sh.mesh_seq, "ext": ext})  # (the very array of the Dirichlet row: assemble() finds the row by it)
        _codim_keywords(cfg, sh, f"shape {s_index} ({os.path.basename(sh.path)})", V, T, SF, E, off, p)
        if is_codim:  # (an elastic shell or rod needs nobody to hold it: it counts as moved)
            elastic = sh.shell_thickness is not None or sh.rod_radius is not None
            p.codim.append((np.arange(off, off + V.shape[0], dtype=np.int32), SF + off,
                            sh.lin_vel is not None or sh.ang_vel_deg is not None or sh.mesh_seq is not None or elastic, E + off))
        p.CEs.append(E + off)
        p.Vs.append(V)
        p.Ts.append(T + off)
        p.SFs.append(SF + off)
        p.nr.append(off + V.shape[0])
        p.tr.append(p.tr[-1] + T.shape[0])
    return p


def _add_mesh_obstacles(cfg, p):
    """kinematic mesh obstacles (MeshCO::MeshCO, MeshCO.cpp:37-58): centred on the vertex mean, rotated, scaled so that the largest
    bounding-box extent equals `scale`, moved to `origin`.  They ride along as surface-only components: nodes of no tetrahedron.  -> their node ids"""
    obstacles = []
    for path, origin, scale, _mu, rot in cfg.mesh_cos:
        Vo, Fo = read_obj(path)
        Vo = Vo - Vo.mean(0)
        Vo = Vo @ _rot(rot).T
        Vo = Vo * (scale / (Vo.max(0) - Vo.min(0)).max()) + origin
        off = p.nr[-1]
        obstacles.append(np.arange(off, off + Vo.shape[0], dtype=np.int32))
        p.Vs.append(Vo)
        p.SFs.append(Fo + off)
        p.nr.append(off + Vo.shape[0])
        p.tr.append(p.tr[-1])
    return obstacles


def _fiber_payload(cfg, tet_ranges):
    """the `fiber` keywords of the shapes as SceneData.fibers holds them: the direction follows the shape line's transform R (p * scale), as a material
    line of the mesh file does; one activation group per fibred shape"""
    out = []
    for s, sh in enumerate(cfg.shapes):
        if sh.fiber is None or tet_ranges[s + 1] <= tet_ranges[s]:
            continue
        if len(out) >= 64:
            raise ValueError("fiber: at most 64 shapes may carry fibres (one activation group each)")
        d = _rot(sh.rotate_deg) @ (np.asarray(sh.fiber["dir"], dtype=np.float64) * sh.scale)
        out.append({"tet_range": (tet_ranges[s], tet_ranges[s + 1]), "dir": d / np.linalg.norm(d), "k": sh.fiber["k"], "law": sh.fiber["law"], "k2": sh.fiber["k2"],
                    "tension_only": sh.fiber["tension_only"], "group": len(out), "act": sh.fiber["act"], "ramp": sh.fiber["ramp"]})
    return out or None


def _start_positions(cfg, V, nSim):
    """`rotateModel` and `size` on the simulated mesh V[:nSim] (in place) -> the start positions where they differ from the rest shape, else None"""
    V0 = None
    if cfg.rot_deg != 0.0 and nSim:
        # main.cpp:1115-1139: the START positions are the model turned about an axis (Eigen::AngleAxis::toRotationMatrix, the axis as
        # given) through `center` = HALF THE EXTENT of the bounding box (not its middle); the rest shape stays as assembled
        c, sn = math.cos(math.radians(cfg.rot_deg)), math.sin(math.radians(cfg.rot_deg))
        ax = np.array(cfg.rot_axis, float)
        R = (1 - c) * np.outer(ax, ax) + c * np.eye(3) + sn * np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        V0 = V.copy()
        center = (V[:nSim].max(0) - V[:nSim].min(0)) / 2.0
        V0[:nSim] = (V[:nSim] - center) @ R.T + center
    if cfg.size > 0 and nSim:
        # main.cpp:1140-1145: the assembled model (all shapes, not the collision objects) is scaled so that the largest
        # bounding-box extent of its start positions equals `size`, then moved so that the box's lower corner sits at the origin
        U = V if V0 is None else V0
        ext = (U[:nSim].max(0) - U[:nSim].min(0)).max()
        V[:nSim] *= cfg.size / ext
        if V0 is not None:
            V0[:nSim] *= cfg.size / ext
        lo = U[:nSim].min(0).copy()
        V[:nSim] -= lo
        if V0 is not None:
            V0[:nSim] -= lo
    return V0


def _codim_masses(cfg, m, T):
    """the nodes of the components without tetrahedra and their lumped masses from the rest shape as it is NOW (see anim_script.lift_at_start), or None, None"""
    if not m.codim:
        return None, None
    V, mass = m.V, np.zeros(m.V.shape[0])
    for ids, tri, _moved, seg in m.codim:
        if len(tri):  # barycentric lumping of the triangle areas times the density (Mesh.cpp:318-343, 399)
            a = 0.5 * np.linalg.norm(np.cross(V[tri[:, 1]] - V[tri[:, 0]], V[tri[:, 2]] - V[tri[:, 0]]), axis=1)
            for k in range(3):
                np.add.at(mass, tri[:, k], cfg.rho * a / 3.0)
        elif len(seg):  # both ends of a segment of length l get density * l^3 pi / 12 (Mesh.cpp:279-295, 399)
            l = np.linalg.norm(V[seg[:, 0]] - V[seg[:, 1]], axis=1)
            for k in range(2):
                np.add.at(mass, seg[:, k], cfg.rho * l ** 3 * math.pi / 12.0)
        else:
            # a point carries the mean nodal mass of the tetrahedral components (avgNodeMass(dim), Mesh.cpp:403-411, 583-607): lumped
            # masses = density * a quarter of the adjacent element volumes
            tm = np.zeros(V.shape[0])
            if T.shape[0]:
                vol = np.abs(np.einsum("ij,ij->i", np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]), V[T[:, 3]] - V[T[:, 0]])) / 6.0
                for k in range(4):
                    np.add.at(tm, T[:, k], cfg.rho * vol / 4.0)
            n_tet_nodes = sum(m.node_ranges[c + 1] - m.node_ranges[c] for c in range(m.n_shapes) if m.has_tets(c))
            mass[ids] = tm.sum() / n_tet_nodes if n_tet_nodes else 0.0
    nodes = np.concatenate([ids for ids, _f, _m, _e in m.codim])
    return nodes, mass[nodes]


def _per(records, value, dtype=np.float64):
    """one value per primitive: value(record) repeated over the primitives record[0] of every record"""
    return np.concatenate([np.full(len(r[0]), value(r), dtype=dtype) for r in records])


def _codim_payloads(p, attachments, V):
    """-> (shell, rod, attachments, chambers, aero) as AssembledScene holds them and apply() hands them on, None where no shape asks for one"""
    shell = rod = chambers = aero = None
    if p.shells:
        if len({r[2] for r in p.shells}) > 1:
            raise ValueError("one bend scale per scene: the shell shapes give different ones")
        shell = {"tri": np.vstack([r[0] for r in p.shells]).astype(np.int32), "thickness": _per(p.shells, lambda r: float(r[1])),
                 "rho": _per(p.shells, lambda r: float(r[3][0])), "YM": _per(p.shells, lambda r: float(r[3][1])), "PR": _per(p.shells, lambda r: float(r[3][2])),
                 "bend": float(p.shells[0][2])}
        if any(r[4][0] > 0.0 for r in p.shells):  # per triangle, as Context.set_shell_strain_limit takes them; a shape without `limit` stays unlimited (0)
            for k, name in enumerate(("limit", "onset", "stiff")):
                shell[name] = _per(p.shells, lambda r: float(r[4][k]))
        if any(r[5][0] for r in p.shells):  # per triangle, as Context.set_shell_membrane takes them; a shape without `rubber` stays StVK (0)
            shell["model"] = _per(p.shells, lambda r: r[5][0], dtype=np.int32)
            shell["alpha"] = _per(p.shells, lambda r: float(r[5][1]))
        if any(r[7] is not None for r in p.shells):  # per triangle, as Context.set_shell_weave takes them; a shape without `weave` stays as it is (0; the rest is not read there)
            wv = lambda k, none: (lambda r: none if r[7] is None else float(r[7][k]))
            shell["weave"] = {"woven": _per(p.shells, lambda r: int(r[7] is not None), dtype=np.int32),
                              "dir": np.vstack([np.tile(np.zeros(3) if r[7] is None else r[7]["dir"], (len(r[0]), 1)) for r in p.shells]),
                              "E1": _per(p.shells, wv("E1", 0.0)), "E2": _per(p.shells, wv("E2", 0.0)), "G12": _per(p.shells, wv("G12", 0.0)),
                              "nu12": _per(p.shells, wv("nu12", 0.0)), "bend_warp": _per(p.shells, wv("bendwarp", 1.0)), "bend_weft": _per(p.shells, wv("bendweft", 1.0))}
        if any(r[6] is not None for r in p.shells):  # per plastic shape its triangle range within the shell and the four parameters, as Context.shell_set_plasticity takes them
            ends = np.cumsum([len(r[0]) for r in p.shells])
            shell["plastic"] = [((int(e - len(r[0])), int(e)),) + tuple(r[6]) for r, e in zip(p.shells, ends) if r[6] is not None]
    if p.rods:
        if len({r[2] for r in p.rods}) > 1:
            raise ValueError("one bend scale per scene: the rod shapes give different ones")
        rod = {"seg": np.vstack([r[0] for r in p.rods]).astype(np.int32), "radius": _per(p.rods, lambda r: float(r[1])),
               "rho": _per(p.rods, lambda r: float(r[3][0])), "YM": _per(p.rods, lambda r: float(r[3][1])), "bend": float(p.rods[0][2])}
    if attachments is not None:  # (`stitch ... rest`: the distance in the rest shape as the stepper gets it, behind `size`)
        r = attachments.pop("rest")
        attachments["L"][r] = np.linalg.norm(V[attachments["nodesA"][r]] - V[attachments["nodesB"][r]], axis=1)
    if p.chambers:
        chambers = {"tri_lists": [q[0].astype(np.int32) for q in p.chambers], "pressure": np.array([q[1] for q in p.chambers], dtype=np.float64),
                    "ramp": np.array([q[2] for q in p.chambers], dtype=np.float64)}
        if any(q[3][0] for q in p.chambers):
            chambers.update(gas=np.array([q[3][0] for q in p.chambers], dtype=bool), ambient=np.array([q[3][1] for q in p.chambers], dtype=np.float64),
                            gamma=np.array([q[3][2] for q in p.chambers], dtype=np.float64))
    if p.aero:
        aero = {"tri_lists": [q[0].astype(np.int32) for q in p.aero], "cn": np.array([q[1] for q in p.aero], dtype=np.float64),
                "ct": np.array([q[2] for q in p.aero], dtype=np.float64), "one_sided": np.array([q[3] for q in p.aero], dtype=bool)}
    return shell, rod, attachments, chambers, aero


def assemble(cfg, read_mesh):
    """main.cpp:880-1198 and AnimScripter::initAnimScript: the shapes become one mesh, the script (anim_script.SETUP) sets up what it holds and moves.  The
    ORDER of the steps is behaviour: see anim_script.lift_at_start, and `rest` of a stitch is measured behind `size`."""
    p = _assemble_shapes(cfg, read_mesh)
    attachments = _attachments(cfg, p.Vs, p.nr)
    obstacles = _add_mesh_obstacles(cfg, p)
    V, T, SF = np.vstack(p.Vs), np.vstack(p.Ts).astype(np.int32), np.vstack(p.SFs).astype(np.int32)
    nSim = p.nr[len(cfg.shapes)]  # the simulated mesh: everything before the obstacle components
    model = _anim.Model(V, _start_positions(cfg, V, nSim), nSim, p.nr, p.tr, len(cfg.shapes), p.codim, obstacles, cfg.handle_ratio)
    _anim.lift_at_start(cfg, model)
    codim_nodes, codim_mass = _codim_masses(cfg, model, T)
    _anim.check_codim_moved(cfg, model)  # (before the refusals of the scripts themselves)
    st = _anim.SETUP[cfg.script](cfg, model, p.given)
    vel = _anim.start_velocity(cfg, model, st.dirichlet)
    sc = AssembledScene(cfg, V, T, SF, p.nr, p.tr, st.dirichlet, vel, st.neumann, np.concatenate(obstacles) if obstacles else None, st.release,
                        codim_nodes, codim_mass, st.codim_fixed, model.V0)
    sc.motions, sc.mesh_i = st.motions, st.mesh_i
    sc.codim_edges = np.vstack(p.CEs).astype(np.int32) if p.CEs else np.zeros((0, 2), dtype=np.int32)
    sc.shell, sc.rod, sc.attachments, sc.chambers, aero = _codim_payloads(p, attachments, V)
    if aero is not None:
        sc.aero = aero
    fibers = _fiber_payload(cfg, sc.tet_ranges)
    if fibers is not None:
        sc.fibers = fibers
    for q in st.seqs:  # the group a sequence drives = the entry of `dirichlet` that holds its nodes
        q["group"] = next(g for g, d in enumerate(st.dirichlet) if d[0] is q["ids"])
    sc.mesh_seqs = st.seqs
    return sc


def apply(sc, be):
    """Drive a backend (the ctypes `Context` of ipc_amd/lib.py, or an adapter over the oracle with the same method names)."""
    cfg = sc.cfg
    be.set_mesh(sc.V, sc.T, YM=cfg.YM, PR=cfg.PR, density=cfg.rho)
    if hasattr(be, "set_components"):
        # the components of the system report (compVAccSize / compFAccSize, main.cpp:1111-1112): the shapes in script order, then every mesh
        # collision object as a component of its own (they are not part of the reference's Mesh<3>: its files end with the last shape)
        be.set_components(sc.node_ranges[1:], sc.tet_ranges[1:])
    groups = cfg.contact_group_tables(len(sc.node_ranges) - 1)
    if groups is not None:
        be.set_contact_groups(groups[0], groups[1], groups[2])
    if sc.codim_nodes is not None:
        be.set_codim_nodes(sc.codim_nodes, sc.codim_mass)
    if sc.shell is not None:  # after set_codim_nodes (it replaces the area masses of its nodes), before opt_init and the pattern
        q = sc.shell
        be.set_shell(q["tri"], q["thickness"], q["YM"], q["PR"], q["rho"], q["bend"])
        if "model" in q:
            be.set_shell_membrane(q["model"], q["alpha"])
        if "weave" in q:
            w = q["weave"]
            be.set_shell_weave(w["woven"], w["dir"], w["E1"], w["E2"], w["G12"], w["nu12"], w["bend_warp"], w["bend_weft"])
        if "limit" in q:
            be.set_shell_strain_limit(q["limit"], q["onset"], q["stiff"])
        for rng, y, yb, creep, harden in q.get("plastic", ()):  # one call per plastic shape, over its triangle range
            be.shell_set_plasticity(rng, y, yb, creep, harden)
    if sc.rod is not None:  # after set_codim_nodes and set_shell (it replaces the segment masses of its nodes), before opt_init and the pattern
        q = sc.rod
        be.set_rod(q["seg"], q["radius"], q["YM"], q["rho"], q["bend"])
    if sc.attachments is not None:  # every `attach` and `stitch` line in one call, behind set_shell / set_rod, before opt_init and the pattern
        q = sc.attachments
        be.set_attachments(q["nodesA"], q["nodesB"], q["k"], q["L"])
    if sc.chambers is not None:  # every `pressure` shape in one call, behind set_shell, before opt_init and the pattern
        be.set_chambers(sc.chambers["tri_lists"], sc.chambers["pressure"])
        if "gas" in sc.chambers:
            be.chamber_set_gas(sc.chambers["gas"], sc.chambers["ambient"], sc.chambers["gamma"])
    if sc.aero is not None:  # every `aero` shape in one call, behind set_shell, before opt_init and the pattern; then the scene's `wind` line
        be.set_aero(sc.aero["tri_lists"], sc.aero["cn"], sc.aero["ct"], sc.aero["one_sided"])
        be.aero_set_wind(cfg.wind, cfg.air_density)
    be.set_energy_type(cfg.energy)
    for s, sh in enumerate(cfg.shapes):
        # (a shell shape's `material` went into set_shell, which sets the masses of its nodes itself: the component call would scale them by rho / density
        # once more, and it has no tetrahedra whose Lame parameters it could set)
        # (the same holds for a rod shape and set_rod)
        if sh.material is not None and all(np.isfinite(sh.material)) and sh.shell_thickness is None and sh.rod_radius is None:
            be.set_component_material((sc.node_ranges[s], sc.node_ranges[s + 1]), (sc.tet_ranges[s], sc.tet_ranges[s + 1]), *sh.material)
    for s, sh in enumerate(cfg.shapes):  # per component, behind the materials
        if sh.plastic is not None and sc.tet_ranges[s + 1] > sc.tet_ranges[s]:
            be.set_plasticity((sc.tet_ranges[s], sc.tet_ranges[s + 1]), *sh.plastic)
    for f in sc.fibers or []:  # per component, behind the materials; a ramped activation starts at 0 (tools/run_scene.py raises it before each step)
        be.set_fibers(f["tet_range"], f["dir"], f["k"], law=f["law"], k2=f["k2"], tension_only=f["tension_only"], group=f["group"])
        if f["act"] != 0.0 and not f["ramp"] > 0.0:
            be.fiber_set_activation(f["group"], f["act"])
    if sc.V0 is not None:
        be.set_positions(sc.V0)
    be.opt_init(cfg.dt, cfg.gravity)
    if cfg.time_integration == "NM":
        be.set_time_integration("NM", cfg.beta, cfg.gamma)
    if sc.codim_edges is not None and len(sc.codim_edges):
        be.set_surface(sc.SF, sc.codim_edges)
    else:
        be.set_surface(sc.SF)
    if sc.codim_fixed is not None:
        be.set_dbc(sc.codim_fixed, 2)
    self_fric = cfg.effective_self_fric()  # (selfFric itself in a scene without `contactFric`)
    fric_scales = None
    if sc.obstacle_nodes is not None:
        # static obstacle: all of its nodes are ZERO Dirichlet nodes; without `selfCollisionOn` only pairs that involve the
        # obstacle collide.
        be.set_dbc(sc.obstacle_nodes, 1)
        be.set_obstacle(sc.obstacle_nodes, obstacle_only=not cfg.self_collision)
        # MeshCO::friction is read (Config.cpp:459-474) and stored, but no friction term is ever evaluated for a mesh collision object:
        # Optimizer::computeEnergyVal / computeGradient / computePrecondMtr add friction for the analytic objects and for the
        # self-collision set only (Optimizer.cpp:3357-3376, 3473-3510, 3676-3705); the value merely switches the lagging loop on
        # (:156-161).  Seen in a run of the reference-compiled code (cubeCliffCO.txt with and without the coefficient).  So pairs that
        # involve an obstacle node carry no friction, the others selfFric.
        self_fric = self_fric if cfg.self_collision else 0.0
        if self_fric > 0:
            fric_scales = (1.0, 0.0)
    if cfg.self_collision or sc.obstacle_nodes is not None:
        be.enable_self_collision(cfg.dHat_eps)
    for origin, normal, mu in cfg.half_spaces:
        idx = be.add_half_space(origin, normal, cfg.dHat_eps)
        if mu > 0:
            be.set_half_space_friction(idx, mu)
    for rc in cfg.round_colliders:  # analytic spheres and capsules, right after the planes
        idx = be.add_round_collider(rc["p0"], rc["p1"], rc["R"], rc["hollow"], cfg.dHat_eps)
        if rc["friction"] > 0:
            be.set_round_collider_friction(idx, rc["friction"])
    plane_fric = any(mu > 0 for *_, mu in cfg.half_spaces) or any(rc["friction"] > 0 for rc in cfg.round_colliders)
    # Optimizer.cpp:146-166: solveFric is true as soon as ANY collision object -- a mesh collision object included -- or selfFric carries a
    # coefficient: the lagging loop with its tangent-space convergence solve then runs even when no pair carries friction
    loop_only = any(mc[3] > 0 for mc in cfg.mesh_cos) and not (self_fric > 0 or plane_fric)
    if self_fric > 0 or plane_fric or loop_only:
        be.set_friction(self_fric, cfg.fric_iter_amt, cfg.eps_v)
        if cfg.eps_v_target > 0 and cfg.eps_v_target != cfg.eps_v:
            be.set_friction_target(cfg.eps_v_target)
        if sc.obstacle_nodes is not None and fric_scales is not None:
            be.set_friction_scales(*fric_scales)
        if loop_only:
            be.force_friction_loop(True)
    if cfg.use_abs_parameters or cfg.dtol_rel != 1e-9 or cfg.kappa_min_multiplier != 1e11:
        be.set_parameter_scaling(cfg.use_abs_parameters, cfg.dtol_rel, cfg.kappa_min_multiplier)
    if cfg.kappa > 0:
        be.set_kappa(cfg.kappa)
    if 0 < cfg.dHat_target < cfg.dHat_eps:
        be.set_dhat_target(cfg.dHat_target)
    if cfg.damping_stiff > 0:
        be.set_damping(cfg.damping_stiff)
    for g, (ids, lin, ang, t0, t1) in enumerate(sc.dirichlet):
        t0, t1 = max(t0, cfg.dbc_time_range[0]), min(t1, cfg.dbc_time_range[1])  # a group acts where its own range and the scene's overlap
        be.add_dirichlet(ids, lin_vel=lin, ang_vel_deg=ang, t0=t0, t1=t1)
        if sc.motions is not None:
            be.set_dirichlet_motion(g, lin_vel=sc.motions[g][0], ang_vel_deg=sc.motions[g][1], center=sc.motions[g][2], force_nonzero=True)
    for ids, acc, t0, t1 in sc.neumann:
        be.add_neumann(ids, acc, t0=max(t0, cfg.nbc_time_range[0]), t1=min(t1, cfg.nbc_time_range[1]))
    if cfg.script == "twist":
        left, right = _scene.border_verts(sc.V, cfg.handle_ratio)
        be.set_twist(left, right)
    if np.any(sc.velocity):
        be.set_velocity(sc.velocity)
    if cfg.warm_start:
        be.set_warm_start(cfg.warm_start)
    be.set_rel_tol(cfg.tol)
    if cfg.restart:
        be.load_status(cfg.restart)
    be.precompute()
    return be


class ReportWriter:
    """The reference's system report files (Optimizer.cpp:488-506, 1497-1512, 1801-1816): `sysE.txt`, `sysM.txt`, `sysL.txt` in `folder`, one line per
    call of write() -- after precompute() and after every time step.  Values in the reference's order (components in sequence, a component's x y z
    adjacent), space separated; the digits are `%.17g`, which reads back to the same doubles, not the reference's 6 significant digits."""

    def __init__(self, folder):
        os.makedirs(folder, exist_ok=True)
        self.paths = {k: os.path.join(folder, f"sys{k}.txt") for k in "EML"}
        for p in self.paths.values():
            open(p, "w").close()

    def write(self, be):
        for k, a in zip("EML", be.system_report()):
            with open(self.paths[k], "a") as f:
                f.write(" ".join("%.17g" % x for x in np.asarray(a, dtype=np.float64).ravel()) + "\n")


class ContactReportWriter:
    """`contact.txt` in `folder` (tools/run_scene.py --contact-report): one line per row of `contact_report()` per call of write() --
    `step a b nPP nPE nPT nEE nMoll argmin minD2 FA.. FB.. TA.. TB.. RA.. RB.. W`, 29 columns, doubles as `%.17g` (they read back to the same doubles).  A row
    is a pair of components `(a, b)` or a component and half-space `(a, -1 - h)`; see `ipcgpu_contact_report` in include/ipcgpu.h.  The reference logs only
    the smallest distance of a converged solve (Optimizer.cpp:2402-2442) and per-object counts (:3070-3087).
    The report is taken on the sets the stepper HOLDS when solve_timestep returns and changes no state, so a run with the writer takes the steps of a run
    without it.  Those sets are the ones of the final positions: with contact on, every trial of a line search rebuilds them at the trial positions
    (HipOptimizer::lineSearch -> computeConstraintSets), at the step's current dHat, and nothing moves between the last line search and the return; the converged
    pass only evaluates the gradient.  The friction set is NOT the one the solve balanced: when a sub-problem has converged, HipOptimizer::nextSubproblem lags
    friction anew at the converged positions before it decides whether another sub-problem follows, so the lag held at the return was taken at the FINAL
    positions.  RA, RB and W are the forces of that fresh lag (the normal forces and tangent frames of the end of the step) over the step's motion from
    `x_prev` -- an estimate of the friction acting at the end of the step, not the terms of the step's last Newton solve.  `self_fric`: the scene's selfFric,
    the coefficient the lagged terms are scaled with (0: no friction columns)."""

    COLUMNS = ("a", "b", "nPP", "nPE", "nPT", "nEE", "nMollified", "argmin")

    def __init__(self, folder, self_fric=0.0):
        os.makedirs(folder, exist_ok=True)
        self.self_fric = self_fric
        self.path = os.path.join(folder, "contact.txt")
        open(self.path, "w").close()

    def write(self, be, step, x_prev=None):
        rows = be.contact_report(x_prev=x_prev if self.self_fric > 0 else None, coef=self.self_fric)
        with open(self.path, "a") as f:
            for r in rows:
                vals = [float(r["minD2"])] + [float(v) for k in ("FA", "FB", "TA", "TB", "RA", "RB") for v in r[k]] + [float(r["W"])]
                f.write(" ".join([str(int(step))] + [str(int(r[k])) for k in self.COLUMNS] + ["%.17g" % v for v in vals]) + "\n")
        return len(rows)


class FieldsWriter:
    """`fields<N>.vtu` files in `folder` (tools/run_scene.py --fields): an ASCII VTK unstructured grid of the tetrahedra at the state the backend holds.
    Cell data: `stress` (Cauchy, six components XX YY ZZ XY YZ XZ), `von_mises`, `J` -- the element records of `elastic_stress()` -- and, only when a shape carries `plastic`, `plasticStrain` (the accumulated plastic strain alpha); only when a shape carries `fiber`, `fiberStretch` (l; 1 without a fibre) and `fiberDir` (the current direction t; 0 0 0 without one).  Point data: the nodal
    `stress` (rest-volume-weighted mean of the incident elements), `von_mises` of that mean, `velocity`; with self-contact on, `contact_force` -- minus the
    barrier gradient of the constraint set rebuilt at these positions with the step's dHat and kappa, Dirichlet rows kept -- and, when the lagged friction
    set is not empty, `friction_force` -- minus the lagged friction gradient of the step from `x_prev` to here.  The reference writes no such file.
    The stress call changes no state.  The two force fields do: `contact_build` replaces the context's constraint set by the one of the written positions, and the
    gradient calls use the stepper's gradient and line-search buffers as scratch.  Every time step rebuilds the set and both buffers before it reads them, so a run
    with the writer takes the steps of a run without it (tests/test_gpu_fields_tool.py) -- except under `warmStart 5`, whose first iterate reads the set the previous
    step left."""

    def __init__(self, folder, sc, contact=False, self_fric=0.0):
        from . import vtu_io
        os.makedirs(folder, exist_ok=True)
        self.folder, self.sc, self.contact, self.self_fric, self._io = folder, sc, contact, self_fric, vtu_io

    def write(self, be, step, x_prev=None):
        elem, node, n_invalid = be.elastic_stress()
        X = np.asarray(be.get_positions())
        nV = X.shape[0]
        cell = {"stress": elem[:, :6], "von_mises": elem[:, 6], "J": elem[:, 7]}
        point = {"stress": node[:, :6], "von_mises": node[:, 6], "velocity": be.kinematics()["velocity"].reshape(nV, 3)}
        if any(sh.plastic is not None for sh in self.sc.cfg.shapes):  # the accumulated plastic strain, only where a shape is plastic: other files are what they were
            cell["plasticStrain"] = be.plastic_get()["alpha"]
        if self.sc.fibers:  # the fibre stretch and the current fibre direction, only where a shape carries `fiber`: other files are what they were
            fs = be.fiber_state()[0]
            cell["fiberStretch"], cell["fiberDir"] = fs[:, 0], fs[:, 2:5]
        if self.contact:
            fs = be.friction_state()  # (the lagged set first: rebuilding the constraint set below is not to touch what it is read from)
            fric = np.zeros((nV, 3))
            if self.self_fric > 0 and x_prev is not None and fs["n_lagged"] > 0 and fs["fricDHat"] > 0:
                fric = -be.friction_gradient_add(x_prev, fs["fricDHat"], self.self_fric).reshape(nV, 3)
            st = be.state()
            be.contact_build(st["dHat"])
            point["contact_force"] = -be.contact_gradient_add(st["dHat"], st["kappa"], projectDBC=False).reshape(nV, 3)
            point["friction_force"] = fric
        path = os.path.join(self.folder, f"fields{step}.vtu")
        self._io.write_vtu(path, X, self.sc.T, cell, point)
        return path, n_invalid
