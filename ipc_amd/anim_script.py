"""The reference's hard-coded scripts (src/AnimScripter.cpp) restated: what `script <name>` sets up on the assembled model (initAnimScript) and what it decides
from the state before each time step (stepAnimScript).  scene_script.assemble() builds the `Model`, calls `SETUP[name]` and `start_velocity`;
AssembledScene.before_step() dispatches through `RULES`.

Every set-up function is `(cfg, model, from_shapes) -> ScriptSetup`: `from_shapes` holds what the shapes' own keywords gave, and the function returns it with
the fields replaced that the script replaces -- a field it does not name stays as the shapes gave it.  A script has exactly one set-up function; none reads
what another one left.  The dictionaries in `release` are the state of the per-step rules, `RULES[kind]` is `(scene, r, be, x, t) -> bool` (True: the backend
was told something)."""
from dataclasses import dataclass, field, replace
import math

import numpy as np

from . import scene as _scene


class UnsupportedKeyword(ValueError):
    pass


# The hard-coded scripts of AnimScripter that move whole components (set-up AnimScripter.cpp:1060-1300, per step :1961-2135): how many
# leading components they move and with what.  Linear velocities in units / s, angular velocities in rad / s about x, y, z.
_S6 = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
_HP = math.pi / 2.0
DCO_SCRIPTS = {
    "DCOSquash": {"n": 2, "lin": _S6[:2]},  # two plates closing along x, turning round when 0.1 apart (:1172-1191, 2034-2051)
    "DCOSquash6": {"n": 6, "lin": _S6},  # six plates closing along x, y, z (the trash compactor; :1193-1221, 2053-2074)
    "DCORotCylinders": {"n": 4, "ang": [(_HP, 0, 0), (-_HP, 0, 0), (0, 0, -_HP), (0, 0, _HP)]},  # :1060-1086, 1961-1975
    "DCOVerschoorRoller": {"n": 6, "ang": [(0, 0, -4.0), (0, 0, -2.0), (0, 0, 2.0), (0, 0, 4.0), (2.0, 0, 0), (-2.0, 0, 0)]},  # :1088-1118, 1977-1991
    "DCOSqueezeOut": {"n": 0},  # every surface-only component is held (the rule of :2102-2124 that would move the first one never fires, see _dco_squeeze_out)
}


# scripts that pick their Dirichlet / Neumann nodes from the bounding box of the assembled mesh (set-up in AnimScripter::initAnimScript)
HANDLE_SCRIPTS = ("fixLowerHalf", "pushRightMost1", "utopiaComparison", "DCOSegBedSquash", "hangLeft")
# nodes picked by a box rule of the start positions and HELD (ZERO: taken out of the system; NONZERO: a Dirichlet set that does not move), or moved
# at a constant velocity (AnimScripter.cpp:153-189, 224-247, 284-297, 318-373, 459-473, 502-516, 790-807, 860-893; per step :1536-1551, 1597-1603,
# 1817-1826); `drop`, `leftHitRight`, `XYRotate` only give start velocities (:853-858, 1336-1374)
HOLD_SCRIPTS = ("hang", "hang2", "hangTopLeft", "stamp", "stampTopLeft", "stampBoth", "stand", "topbottomfix", "corner", "fixRightMost1")
PULL_SCRIPTS = ("stretch", "squash", "dragdown", "curtain")
INITVEL_SCRIPTS = ("drop", "leftHitRight", "XYRotate")
# handle sets that move, turn round or stop by a rule on one "turning" node (AnimScripter.cpp:375-457, 518-553, 574-631; per step :1554-1595, 1648-1729)
TURN_SCRIPTS = ("push", "tear", "upndown", "undstamp", "stretchnsquash", "bend")
TWIST_SCRIPTS = ("twistnstretch", "twistnsns", "twistnsns_old")
# handle sets that are LET GO (the others stop) when the turning node has travelled far enough (:633-760, 827-851; per step :1731-1812)
LET_GO_SCRIPTS = ("rubberBandPull", "fourLegPull", "headTailPull", "toggleTop")
# start positions changed and / or nodes held (:129-151, 206-222, 265-282, 299-316), Neumann pull on the top (:912-954)
START_SCRIPTS = ("scaleF", "swing", "stampInv", "standInv", "NMFixBottomDragLeft", "NMFixBottomDragForward")
RULE_SCRIPTS = TURN_SCRIPTS + TWIST_SCRIPTS + LET_GO_SCRIPTS + START_SCRIPTS
# scripts that hold or move the components without tetrahedra themselves; under any other one each of them needs keywords of its own that move it
CODIM_SCRIPTS = tuple(DCO_SCRIPTS) + ("DCOFix", "DCOBallHitWall", "DCOSegBedSquash", "meshSeqFromFile", "DCOHammerWalnut", "DCOCut")

ZERO3 = (0.0, 0.0, 0.0)
INF = float("inf")


@dataclass
class Model:
    """The assembled model as the scripts see it (mesh.V of the reference is `start()`; the scripts read and WRITE it in place)."""
    V: np.ndarray  # the rest shape
    V0: np.ndarray  # start positions where they differ from it (`rotateModel`, and the scripts that change them), else None
    nSim: int  # the simulated mesh: every node before the mesh collision objects
    node_ranges: list
    tet_ranges: list
    n_shapes: int
    codim: list  # (node ids, triangles, moved by its own keywords, segments) of the components without tetrahedra
    obstacles: list  # node ids of every mesh collision object
    handle_ratio: float = 0.01

    def start(self):
        return self.V if self.V0 is None else self.V0

    def sim(self):
        return self.start()[:self.nSim]

    def own_start(self):
        """start positions that are not the rest shape: a script is about to change them (the rest shape stays)"""
        if self.V0 is None:
            self.V0 = self.V.copy()
        return self.V0

    def box(self, ids=None):
        """lo, hi, hi - lo of the start positions of the simulated mesh (mesh.V.colwise().minCoeff() / maxCoeff()) or of the nodes `ids`"""
        U = self.sim() if ids is None else self.start()[ids]
        lo, hi = U.min(0), U.max(0)
        return lo, hi, hi - lo

    def border(self):
        """the left and the right handle set (mesh.borderVerts_primitive, main.cpp:1180)"""
        return _scene.border_verts(self.sim(), self.handle_ratio)

    @staticmethod
    def ids(mask):
        return np.nonzero(mask)[0].astype(np.int32)

    def component(self, c):
        return np.arange(self.node_ranges[c], self.node_ranges[c + 1], dtype=np.int32)

    def has_tets(self, c):
        return self.tet_ranges[c + 1] > self.tet_ranges[c]

    def lift_half_diagonal(self, rest_too):
        """Mesh<3> only (the obstacles are not part of it in the reference) goes up by half the diagonal of its bounding box.  `fall` and `dragdown` lift
        the rest shape with the start positions; `dragright` lifts mesh.V alone (with `rotateModel` that is not the rest shape -- 13_dolphinFunnel.txt;
        found by running that scene through the reference)."""
        lo, hi, _rng = self.box()
        lift = 0.5 * np.linalg.norm(hi - lo)
        if rest_too or self.V0 is None:
            self.V[:self.nSim, 1] += lift
        if self.V0 is not None:
            self.V0[:self.nSim, 1] += lift


def moved(ids, lin, ang=ZERO3, centre=None):
    """a Dirichlet group of nodes `ids` that moves at `lin` and turns at `ang` (degrees) about `centre` (None: its own, moving, centre)"""
    return ids, lin, ang, centre


def held(ids):
    return moved(ids, ZERO3)


@dataclass
class ScriptSetup:
    """What the shapes' keywords gave and a script may replace (the fields of AssembledScene of the same names)."""
    dirichlet: list = field(default_factory=list)  # (ids, lin_vel, ang_vel_deg, t0, t1)
    neumann: list = field(default_factory=list)  # (ids, acceleration, t0, t1)
    seqs: list = field(default_factory=list)  # mesh sequences: {ids, folder, ext}
    motions: list = None  # per Dirichlet group: (lin, ang in degrees, fixed centre or None) with the nodes typed NONZERO throughout
    release: dict = None  # the state of the script's per-step rule
    codim_fixed: np.ndarray = None
    mesh_i: int = 0

    def with_groups(self, groups, zero=False, **other):
        """resetDBCVertices(): the script's groups (of `moved` / `held`) replace whatever the shapes' own DBC keywords selected.  zero: the nodes are typed
        ZERO (taken out of the system), so no motion is listed."""
        return replace(self, dirichlet=[(ids, lin, ang, 0.0, INF) for ids, lin, ang, _c in groups],
                       motions=None if zero else [(lin, ang, c) for _ids, lin, ang, c in groups], **other)


def _nothing(cfg, m, s):
    return s


def lift_at_start(cfg, m):
    """AnimScripter.cpp:779-792: `fall` and `dragdown` lift the model by half its bounding-box diagonal.  On its own because of its place in the sequence:
    BEFORE the masses of the components without tetrahedra are lumped (areas of lifted triangles round differently); `dragright` lifts behind them."""
    if cfg.script in ("fall", "dragdown"):
        m.lift_half_diagonal(rest_too=True)


def check_codim_moved(cfg, m):
    if m.codim and cfg.script not in CODIM_SCRIPTS and not all(moved_ for _i, _f, moved_, _e in m.codim):
        raise UnsupportedKeyword("codimensional shape that no script fixes or moves")


def _fall(cfg, m, s):  # AnimScripter.cpp:779-788: lifted (fall only, see lift_at_start), no Dirichlet nodes
    return replace(s, dirichlet=[])


def _hold(cfg, m, s):
    U = m.sim()
    lo, hi, rng = m.box()
    left, right = m.border()
    zero = cfg.script in ("hang", "hang2", "hangTopLeft")  # typed ZERO; the others NONZERO
    if cfg.script == "hang":  # the LAST node of either border set
        ids = np.array([b[-1] for b in (left, right) if len(b)], dtype=np.int32)
    elif cfg.script == "hang2":  # the top 1 %
        ids = m.ids(U[:, 1] > hi[1] - rng[1] * 0.01)
    elif cfg.script == "hangTopLeft":  # the nodes of the left border set in the top 1 % and within 1 % of either z end
        L = np.asarray(left)
        ids = L[(U[L, 1] > hi[1] - rng[1] * 0.01) & ((U[L, 2] > hi[2] - rng[2] * 0.01) | (U[L, 2] < lo[2] + rng[2] * 0.01))].astype(np.int32)
    elif cfg.script == "stamp":
        ids = np.asarray(left, dtype=np.int32)
    elif cfg.script == "stampTopLeft":
        L = np.asarray(left)
        ids = L[U[L, 1] > hi[1] - rng[1] * 0.01].astype(np.int32)
    elif cfg.script == "stampBoth":
        ids = np.concatenate([left, right]).astype(np.int32)
    elif cfg.script == "stand":  # the bottom 1 %
        ids = m.ids(U[:, 1] < lo[1] + rng[1] * 0.01)
    elif cfg.script == "topbottomfix":  # the bottom and the top 2 %
        ids = m.ids((U[:, 1] < lo[1] + rng[1] * 0.02) | (U[:, 1] > hi[1] - rng[1] * 0.02))
    elif cfg.script == "corner":  # within 1 % of the x, y or z minimum
        ids = m.ids((U[:, 0] < lo[0] + rng[0] * 0.01) | (U[:, 1] < lo[1] + rng[1] * 0.01) | (U[:, 2] < lo[2] + rng[2] * 0.01))
    else:  # fixRightMost1: the FIRST node within 1e-3 of the right end
        ids = m.ids(U[:, 0] > hi[0] - 1.0e-3 * rng[0])[:1]
    groups = [held(ids)] if len(ids) else []
    return s.with_groups(groups, zero=zero or not groups)


def _pull(cfg, m, s):
    U = m.sim()
    lo, hi, rng = m.box()
    left, right = m.border()
    if cfg.script in ("stretch", "squash"):  # the border sets pulled apart at 0.1 / pushed together at 0.03 along x
        v = -0.1 if cfg.script == "stretch" else 0.03
        groups = [moved(np.asarray(left, dtype=np.int32), (v, 0.0, 0.0)), moved(np.asarray(right, dtype=np.int32), (-v, 0.0, 0.0))]
    elif cfg.script == "dragdown":  # (lifted like `fall`, see lift_at_start) the middle of the bottom tenth pulled down at 1.5
        groups = [moved(m.ids((U[:, 1] < lo[1] + rng[1] * 0.1) & (U[:, 0] < lo[0] + rng[0] * 0.52) & (U[:, 0] > lo[0] + rng[0] * 0.42)), (0.0, -1.5, 0.0))]
    else:  # curtain: eight pins along the top edge, pin i drawn in +x at 0.04 (7 - i) / 7; a node takes the first pin that fits
        groups, taken = [], np.zeros(len(U), dtype=bool)
        for pin in range(8):
            x0 = lo[0] + rng[0] / 7.0 * pin
            mask = (U[:, 0] > x0 - rng[0] * 0.0025) & (U[:, 0] < x0 + rng[0] * 0.0025) & (U[:, 1] > hi[1] - rng[1] * 0.005) & ~taken
            taken |= mask
            groups.append(moved(m.ids(mask), (0.04 * (7.0 - pin) / 7.0, 0.0, 0.0)))
    return s.with_groups([g for g in groups if len(g[0])])


def _drop_empty(groups):
    """the groups that have nodes, and old index -> new index (group indices are positions in `dirichlet`)"""
    keep = [k for k, g in enumerate(groups) if len(g[0])]
    return [groups[k] for k in keep], {k: i for i, k in enumerate(keep)}


def _with_turn(s, groups, turn=None):
    """groups that move until the rule of `turn` = (node, axis, lo, hi, component that changes sign, groups it applies to, stop instead) turns or stops them"""
    groups, remap = _drop_empty(groups)
    s = s.with_groups(groups, zero=not groups)
    if turn is None:
        return s
    return replace(s, release={"kind": "turn", "turn": turn[0], "axis": turn[1], "lo": float(turn[2]), "hi": float(turn[3]), "comp": turn[4],
                               "groups": [remap[g] for g in turn[5] if g in remap], "stop": turn[6], "lin": [q[0] for q in s.motions],
                               "ang": [q[1] for q in s.motions], "ctr": [q[2] for q in s.motions], "done": False})


def _turning(cfg, m, s):
    U = m.sim()
    lo, hi, rng = m.box()
    left, right = m.border()
    turn = None
    if cfg.script in ("push", "tear"):  # bottom 1 % held; top 1 % pushed down at 1 until it is 0.5 lower / dragged in -x at 5, turning at 4 further left
        bottom = U[:, 1] < lo[1] + rng[1] * 0.01
        top = m.ids(~bottom & (U[:, 1] > hi[1] - rng[1] * 0.01))
        groups = [held(m.ids(bottom)), moved(top, (0.0, -1.0, 0.0) if cfg.script == "push" else (-5.0, 0.0, 0.0))]
        if len(top):
            turn = (int(top[0]), 1, U[top[0], 1] - 0.5, np.inf, 1, [1], True) if cfg.script == "push" else (int(top[0]), 0, U[top[0], 0] - 4.0, np.inf, 0, [1], False)
    elif cfg.script in ("upndown", "undstamp"):  # the border sets (undstamp: the left one) go up / down at 1.8, turning 0.6 above and below the start
        sets = [left, right] if cfg.script == "upndown" else [left]
        groups = [moved(b, (0.0, (-1.0) ** i * 1.8, 0.0)) for i, b in enumerate(sets)]
        turn = (int(left[0]), 1, U[left[0], 1] - 0.6, U[left[0], 1] + 0.6, 1, list(range(len(sets))), False)
    elif cfg.script == "stretchnsquash":  # pulled apart at 0.9, turning when the first left node is 0.8 further out / 0.4 further in
        groups = [moved(b, ((-1.0) ** i * -0.9, 0.0, 0.0)) for i, b in enumerate((left, right))]
        turn = (int(left[0]), 0, U[left[0], 0] - 0.8, U[left[0], 0] + 0.4, 0, [0, 1], False)
    else:  # bend: every border node but the last of its set turns about z through that last one at 0.05 pi (9 degrees) per unit time
        groups = []
        for i, b in enumerate((left, right)):
            groups.append(moved(b[:-1], ZERO3, (0.0, 0.0, (-1.0) ** i * -9.0), tuple(U[b[-1]])))
            groups.append(held(b[-1:]))
    return _with_turn(s, groups, turn)


def _twist(cfg, m, s):
    """twist about x through the rest box centre + a pull along x; twistnsns turns the pull round like stretchnsquash"""
    U = m.sim()
    left, right = m.border()
    ctr_rest = tuple(0.5 * (m.V[:m.nSim].min(0) + m.V[:m.nSim].max(0)))  # mesh.bbox.colwise().mean(): the rest shape's box
    w, v, out = {"twistnstretch": (18.0, 0.1, None), "twistnsns": (72.0, 1.2, 1.2), "twistnsns_old": (72.0, 0.9, 0.8)}[cfg.script]
    groups = [moved(b, ((-1.0) ** i * -v, 0.0, 0.0), ((-1.0) ** i * -w, 0.0, 0.0), ctr_rest) for i, b in enumerate((left, right))]
    turn = None if out is None else (int(left[0]), 0, U[left[0], 0] - out, U[left[0], 0] + 0.4, 0, [0, 1], False)
    return _with_turn(s, groups, turn)


def _let_go(cfg, m, s):
    U = m.sim()
    lo, hi, rng = m.box()
    y0, y1, x0, x1, z0, z1 = lo[1], hi[1], lo[0], hi[0], lo[2], hi[2]
    # sets: (mask, velocity, let go?); lim: (set whose first node decides, axis, offset of the limit, "<=")
    if cfg.script == "rubberBandPull":  # bottom / top 2 % drawn apart at 0.2, the waist pulled in -x at 2.5 and let go 5 further left
        a = U[:, 1] < y0 + rng[1] * 0.02
        b = ~a & (U[:, 1] > y1 - rng[1] * 0.02)
        w = ~a & ~b & (U[:, 1] < y1 - rng[1] * 0.48) & (U[:, 1] > y0 + rng[1] * 0.48)
        sets = [(a, (0.0, -0.2, 0.0), False), (b, (0.0, 0.2, 0.0), False), (w, (-2.5, 0.0, 0.0), True)]
        lim = (2, 0, -5.0, True)
    elif cfg.script == "fourLegPull":
        a = (U[:, 1] > y1 - rng[1] * 0.129) & (U[:, 0] < x0 + rng[0] * 0.16)
        b = ~a & (U[:, 1] > y1 - rng[1] * 0.16) & (U[:, 0] > x1 - rng[0] * 0.16)
        c = ~a & ~b & (U[:, 1] < y0 + rng[1] * 0.02) & (U[:, 0] > x1 - rng[0] * 0.25)
        d = ~a & ~b & ~c & (U[:, 1] < y0 + rng[1] * 0.02) & (U[:, 0] < x0 + rng[0] * 0.25)
        sets = [(a, ZERO3, False), (b, (2.5, 0.0, 0.0), True), (c, (2.5, -3.5, 0.0), True), (d, (0.0, -3.5, 0.0), True)]
        lim = (3, 1, -5.0, True)
    elif cfg.script == "headTailPull":
        a = U[:, 2] < z0 + rng[2] * 0.02
        b = ~a & (U[:, 2] > z1 - rng[2] * 0.02)
        c = ~a & ~b & (U[:, 2] > z0 + rng[2] * 0.46) & (U[:, 2] < z0 + rng[2] * 0.54)
        sets = [(a, (3.5, 0.0, 0.0), True), (b, (3.5, 0.0, 0.0), True), (c, ZERO3, False)]
        lim = (0, 0, 4.5, False)
    else:  # toggleTop: the top 2 % drawn in -x at 0.5 and let go 0.1 further left
        sets = [(U[:, 1] > y1 - rng[1] * 0.02, (-0.5, 0.0, 0.0), True)]
        lim = (0, 0, -0.1, True)
    all_groups = [moved(m.ids(mask), lin) for mask, lin, _f in sets]
    groups, remap = _drop_empty(all_groups)
    s = s.with_groups(groups, zero=not groups)
    first = all_groups[lim[0]][0]
    if not len(first):
        return s
    return replace(s, release={"kind": "let_go", "turn": int(first[0]), "axis": lim[1], "limit": float(U[first[0], lim[1]] + lim[2]), "below": lim[3],
                               "free": [remap[k] for k, (_m, _l, f) in enumerate(sets) if f and k in remap],
                               "stop": [remap[k] for k, (_m, _l, f) in enumerate(sets) if not f and k in remap], "done": False})


def _start_changing(cfg, m, s):
    U = m.sim()  # (read before the start positions get a copy of their own: where they were the rest shape, U stays the rest shape)
    lo, hi, rng = m.box()
    if cfg.script == "scaleF":  # every start position times 1.5 about the origin
        m.own_start()[:m.nSim] *= 1.5
        return s.with_groups([], zero=True)
    if cfg.script == "swing":  # lifted by 1.3 heights, the left 5 % held (ZERO)
        m.own_start()[:m.nSim, 1] += 1.3 * rng[1]
        groups, _ = _drop_empty([held(m.ids(U[:, 0] < lo[0] + rng[0] * 0.05))])
        return s.with_groups(groups, zero=True)
    if cfg.script in ("stampInv", "standInv"):  # the left / bottom 1 % held; the start turned inside out and squeezed to a tenth about it
        ax = 0 if cfg.script == "stampInv" else 1
        ids = m.ids(U[:, ax] < lo[ax] + rng[ax] * 0.01)
        off = 1.1 * U[ids[0], ax]  # *mesh.DBCVertexIds.begin(): the smallest held index
        W = m.own_start()
        W[:m.nSim, ax] = -0.1 * W[:m.nSim, ax] + off
        return s.with_groups([held(ids)])
    # NMFixBottomDrag*: the bottom 5 % held, the top 5 % pulled by a Neumann acceleration of 600 in -x / +x
    bottom = U[:, 1] < lo[1] + rng[1] * 0.05
    groups, _ = _drop_empty([held(m.ids(bottom))])
    pull = (m.ids(~bottom & (U[:, 1] > hi[1] - rng[1] * 0.05)), (-600.0 if cfg.script == "NMFixBottomDragLeft" else 600.0, 0.0, 0.0), 0.0, INF)
    return s.with_groups(groups, zero=not groups, neumann=[pull])


def _dragright(cfg, m, s):
    """AnimScripter.cpp:809-826: lifted like `fall` (behind the mass lumping), the nodes within 4 % of the right end of the body become a NONZERO handle
    pulled at 0.5 in +x; stepAnimScript lets go once the whole body is right of every mesh obstacle (:1619-1632)"""
    m.lift_half_diagonal(rest_too=False)
    lo, hi, _rng = m.box()
    ids = m.ids(m.sim()[:, 0] > hi[0] - 0.04 * (hi[0] - lo[0]))
    limit = max((m.V[o, 0].max() for o in m.obstacles), default=-np.inf)
    return replace(s, dirichlet=[(ids, (0.5, 0.0, 0.0), ZERO3, 0.0, INF)], release={"group": 0, "x_limit": float(limit), "nSim": int(m.nSim), "done": False})


def _aco(cfg, m, s):  # AnimScripter.cpp:956-985: no Dirichlet nodes; planes 2 i / 2 i + 1 move at +1 / -1 along axis i
    nP = 2 if cfg.script == "ACOSquash" else 6
    if len(cfg.half_spaces) < nP:
        raise UnsupportedKeyword(f"script {cfg.script} needs {nP} analytic planes (ground / halfSpace)")
    vel_p = [np.eye(3)[i // 2] * (1.0 if i % 2 == 0 else -1.0) for i in range(nP)]
    return replace(s, dirichlet=[], release={"kind": "aco", "vel": vel_p, "origins": [np.array(h[0], dtype=np.float64) for h in cfg.half_spaces[:nP]],
                                             "pairs": [(a, 0.1 if nP == 2 else 0.2) for a in range(0, nP, 2)], "done": False})


def _mesh_seq_from_file(cfg, m, s):
    """AnimScripter.cpp:1222-1236, 2126-2144: every component without tetrahedra is a NONZERO Dirichlet set; before each step the FIRST of them is
    moved onto the positions of <folder>/<meshI>.obj, meshI counted from 1"""
    parts = [ids for ids, _f, _m, _e in m.codim]
    if not parts:
        raise UnsupportedKeyword("script meshSeqFromFile without a surface-only component to move")
    return s.with_groups([held(ids) for ids in parts], seqs=[{"ids": parts[0], "folder": cfg.script_seq_folder, "ext": ".obj"}], mesh_i=1)


def _dco_fix(cfg, m, s):  # AnimScripter.cpp:1222-1236: mesh.resetDBCVertices(); every codimensional component is held (NONZERO, no motion)
    return replace(s, dirichlet=[], codim_fixed=np.concatenate([ids for ids, _f, _m, _e in m.codim]) if m.codim else None)


def _refuse_unheld_surfaces(m, comps):
    if any(not m.has_tets(c) and c not in comps for c in range(m.n_shapes)):
        raise UnsupportedKeyword("surface-only component that the script neither moves nor holds")


def _dco_squeeze_out(cfg, m, s):
    """Every surface-only component is a NONZERO Dirichlet node set (AnimScripter.cpp:1261-1280); the first one carries a velocity of
    0.3 downwards that is applied while `topMax > bottomMin + (bottomMax - bottomMin) / 3.8 * 0.9` (:2102-2124).  As shipped that
    test is never true: bottomMin starts at -infinity and is updated with std::min, so it STAYS -infinity and the right-hand side
    is -inf + inf = NaN.  Seen in a run of the reference-compiled code (the plane does not move); restated as what it does."""
    return s.with_groups([held(m.component(c)) for c in range(m.n_shapes) if not m.has_tets(c)])  # mesh.componentCoDim[compI] < 3


def _dco(cfg, m, s):
    spec = DCO_SCRIPTS[cfg.script]
    n = spec["n"]
    if m.n_shapes < n + 1:
        raise UnsupportedKeyword(f"script {cfg.script} needs {n} scripted components and a body")
    groups = []
    for c in range(n):
        ids = m.component(c)
        lo, hi, _rng = m.box(ids)
        lin = tuple(float(x) for x in spec["lin"][c]) if "lin" in spec else ZERO3
        ang = tuple(math.degrees(x) for x in spec["ang"][c]) if "ang" in spec else ZERO3
        groups.append(moved(ids, lin, ang, tuple(0.5 * (hi + lo)) if "ang" in spec else None))  # MCORotCenter: fixed at set-up
    _refuse_unheld_surfaces(m, range(n))
    return s.with_groups(groups, release={"kind": "dco", "script": cfg.script, "done": False, "lin": [g[1] for g in groups]} if "lin" in spec else None)


def _dco_second(cfg, m, s):
    """AnimScripter.cpp:1120-1170, 1993-2032: the SECOND component (whatever its kind) is a NONZERO set; while its lowest node is above 0.05 it
    turns about z at pi / 6 through (x max, y min, z middle) of its start box (the hammer), resp. above 0.001 it moves at (0, -1, -1) (the knife)"""
    if m.n_shapes < 2:
        raise UnsupportedKeyword(f"script {cfg.script} needs a second component to move")
    ids = m.component(1)
    lo, hi, _rng = m.box(ids)
    if cfg.script == "DCOHammerWalnut":
        mot, y_stop = (ZERO3, (0.0, 0.0, 30.0), (float(hi[0]), float(lo[1]), float(0.5 * (hi[2] + lo[2])))), 0.05
    else:
        mot, y_stop = ((0.0, -1.0, -1.0), ZERO3, None), 0.001
    _refuse_unheld_surfaces(m, (1,))
    return s.with_groups([moved(ids, *mot)], release={"kind": "while_above", "ids": ids, "y": y_stop, "motion": mot, "moving": True, "done": False})


def _stretch_and_pause(cfg, m, s):
    """AnimScripter.cpp:475-500: the nodes within 1 % of the left / right end of the model are NONZERO handles pulled apart at 1 in
    -x / +x; the turning vertex is the LAST left handle in index order (`turningPointAdded` is never set), the limit x = -0.28"""
    U = m.sim()
    lo, hi, _rng = m.box()
    left = m.ids(U[:, 0] < lo[0] + 0.01 * (hi[0] - lo[0]))
    right = m.ids((U[:, 0] > hi[0] - 0.01 * (hi[0] - lo[0])) & ~(U[:, 0] < lo[0] + 0.01 * (hi[0] - lo[0])))
    return replace(s, dirichlet=[(left, (-1.0, 0.0, 0.0), ZERO3, 0.0, INF), (right, (1.0, 0.0, 0.0), ZERO3, 0.0, INF)],
                   release={"kind": "pause", "turn": int(left[-1]), "x_limit": -0.28, "groups": [0, 1], "ids": [left, right], "done": False})


def _handle(cfg, m, s):
    U = m.sim()
    lo, hi, rng = m.box()  # mesh.V.colwise().minCoeff() / maxCoeff(): every node of Mesh<3>
    if cfg.script == "hangLeft":  # AnimScripter.cpp:191-204: the left border nodes (IglUtils::findBorderVerts, handleRatio 0.01) are held (ZERO)
        return s.with_groups([held(np.asarray(m.border()[0], dtype=np.int32))], zero=True)
    if cfg.script == "fixLowerHalf":  # AnimScripter.cpp:337-350: the lower half of the model is held (NONZERO, no motion)
        return s.with_groups([held(m.ids(U[:, 1] < lo[1] + rng[1] * 0.5))])
    if cfg.script == "pushRightMost1":  # :895-910, 1820-1826: the FIRST node within 1e-3 of the right end is pushed at 0.15 in -x
        return s.with_groups([moved(np.nonzero(U[:, 0] > hi[0] - 1.0e-3 * rng[0])[0][:1].astype(np.int32), (-0.15, 0.0, 0.0))])
    # utopiaComparison (:1283-1302, 1641-1646): nodes within 1e-4 of the model's WIDTH (range[0], as written) of the top carry a Neumann acceleration of
    # 1.5 downwards, those as close to the bottom are held
    top = U[:, 1] > hi[1] - rng[0] * 1e-4
    bottom = ~top & (U[:, 1] < lo[1] + rng[0] * 1e-4)
    return s.with_groups([held(m.ids(bottom))], neumann=[(m.ids(top), (0.0, -1.5, 0.0), 0.0, INF)])


def _seg_bed_squash(cfg, m, s):
    """DCOSegBedSquash (:1239-1259, 2080-2100): every component without tetrahedra is a NONZERO Dirichlet set; those in the upper half of
    the component list (index >= (#components + 1) / 2) move down at 1 while the gap between the lowest node of the upper ones and the
    highest node of the lower ones exceeds 0.1 -- the two beds of `17_pinCushionBall.txt` closing on the ball"""
    parts = [c for c in range(m.n_shapes) if not m.has_tets(c)]
    if not parts:
        raise UnsupportedKeyword("script DCOSegBedSquash without a component to move")
    cat = lambda cs: np.concatenate([m.component(c) for c in cs]) if cs else np.zeros(0, np.int32)  # noqa: E731
    up, down = cat([c for c in parts if c >= (m.n_shapes + 1) // 2]), cat([c for c in parts if c < (m.n_shapes + 1) // 2])
    groups, _ = _drop_empty([held(down), moved(up, (0.0, -1.0, 0.0))])
    return s.with_groups(groups, release={"kind": "segbed", "up": up, "down": down, "group": len(groups) - 1, "moving": True, "done": False} if len(up) else None)


SETUP = {
    **{name: _nothing for name in ("null", "twist") + INITVEL_SCRIPTS},  # (`twist`: apply() hands the border sets to the backend; start velocities below)
    "fall": _fall, "fallNoShift": _fall, "dragright": _dragright, "ACOSquash": _aco, "ACOSquash6": _aco, "meshSeqFromFile": _mesh_seq_from_file,
    "DCOFix": _dco_fix, "DCOBallHitWall": _dco_fix, "DCOHammerWalnut": _dco_second, "DCOCut": _dco_second, "stretchAndPause": _stretch_and_pause,
    **{name: _hold for name in HOLD_SCRIPTS}, **{name: _pull for name in PULL_SCRIPTS},
    **{name: _turning for name in TURN_SCRIPTS}, **{name: _twist for name in TWIST_SCRIPTS}, **{name: _let_go for name in LET_GO_SCRIPTS},
    **{name: _start_changing for name in START_SCRIPTS},
    **{name: _dco for name in DCO_SCRIPTS}, "DCOSqueezeOut": _dco_squeeze_out,
    **{name: _handle for name in HANDLE_SCRIPTS}, "DCOSegBedSquash": _seg_bed_squash,
}


def start_velocity(cfg, m, dirichlet):
    """the velocities the nodes start with: `DCOBallHitWall`, the INITVEL_SCRIPTS, and `initVel` on a shape under `script null`"""
    vel = np.zeros_like(m.V)
    if cfg.script == "DCOBallHitWall":  # AnimScripter.cpp:1376-1389: every node of a tetrahedral component starts at v_x (default 1000)
        vx = cfg.script_params[0] if cfg.script_params and cfg.script_params[0] == cfg.script_params[0] else 1000.0
        for c in range(m.n_shapes):
            if m.has_tets(c):
                vel[m.node_ranges[c]:m.node_ranges[c + 1], 0] = vx
    if cfg.script in INITVEL_SCRIPTS:  # AnimScripter::initVelocity (AnimScripter.cpp:1336-1374), over every node of Mesh<3>
        U = m.sim()
        lo, hi, rng = m.box()
        if cfg.script == "drop":
            vel[:m.nSim, 1] = -1.0
        elif cfg.script == "leftHitRight":
            vel[:m.nSim][U[:, 0] < lo[0] + rng[0] / 2.0, 0] = 1.0
        else:
            bottom = U[:, 1] < lo[1] + rng[1] * 0.01
            vel[:m.nSim][bottom, 0] = 1.0
            vel[:m.nSim][~bottom & (U[:, 1] > hi[1] - rng[1] * 0.01), 0] = -1.0
    fixed = np.zeros(m.V.shape[0], dtype=bool)
    for ids, *_ in dirichlet:
        fixed[ids] = True
    for c, sh in enumerate(cfg.shapes):  # AnimScripter::initVelocity (AnimScripter.cpp:1319-1333): `initVel` under `script null` only
        if sh.init_vel is None or cfg.script != "null" or not m.has_tets(c):
            continue
        a, b = m.node_ranges[c], m.node_ranges[c + 1]
        ctr = 0.5 * (m.V[a:b].max(0) + m.V[a:b].min(0))
        v = np.array(sh.init_vel[0]) + np.cross(np.radians(np.array(sh.init_vel[1])), m.V[a:b] - ctr)
        v[fixed[a:b]] = 0.0
        vel[a:b] = v
    return vel


# ---- per step (AnimScripter::stepAnimScript): RULES[kind](scene, r, be, x, t), x the positions the step starts from ----------------------------------------
def _rule_dco(scene, r, be, x, t):
    nr = scene.node_ranges
    if r["script"] in ("DCOSquash", "DCOSquash6"):
        # AnimScripter.cpp:2034-2074: while the first two plates are closer than 0.1 in x, EVERY velocity changes sign -- once per
        # time step, as written
        if x[nr[1]:nr[2], 0].min() - x[nr[0]:nr[1], 0].max() < 0.1:
            r["lin"] = [tuple(-c for c in v) for v in r["lin"]]
            for g, v in enumerate(r["lin"]):
                be.set_dirichlet_motion(g, lin_vel=v, force_nonzero=True)
            return True
    return False


def _rule_segbed(scene, r, be, x, t):  # AnimScripter.cpp:2080-2100: the upper parts move only while they are more than 0.1 above the lower ones
    top_min = x[r["up"], 1].min()
    bottom_max = x[r["down"], 1].max() if len(r["down"]) else -np.inf
    moving = bool(top_min - bottom_max > 0.1)
    if moving == r["moving"]:
        return False
    r["moving"] = moving
    be.set_dirichlet_motion(r["group"], lin_vel=(0.0, -1.0, 0.0) if moving else ZERO3, force_nonzero=True)
    return True


def _rule_turn(scene, r, be, x, t):
    """one node decides (velocityTurningPoints): outside its window the listed velocity components change sign -- every step it is found
    outside, as written (AnimScripter.cpp:1568-1595, 1648-1660, 1702-1729) -- or, `push`, the handles stop for good (:1554-1566)"""
    c = x[r["turn"], r["axis"]]
    if not (c <= r["lo"] or c >= r["hi"]):
        return False
    if r["stop"]:
        r["lin"] = [ZERO3 if g in r["groups"] else v for g, v in enumerate(r["lin"])]
        r["done"] = True
    else:
        r["lin"] = [tuple(-c_ if k == r["comp"] else c_ for k, c_ in enumerate(v)) if g in r["groups"] else v for g, v in enumerate(r["lin"])]
    for g in r["groups"]:
        be.set_dirichlet_motion(g, lin_vel=r["lin"][g], ang_vel_deg=r["ang"][g], center=r["ctr"][g], force_nonzero=True)
    return True


def _rule_aco(scene, r, be, x, t):
    """AnimScripter.cpp:1832-1871: the analytic planes close in at 1 along their axis, every velocity of a pair changing sign while the two
    are closer than 0.1 (ACOSquash) / 0.2 (ACOSquash6); each plane then moves by the fraction of v dt that HalfSpace::move admits"""
    o, v = r["origins"], r["vel"]
    for a, gap in r["pairs"]:
        if o[a + 1][a // 2] - o[a][a // 2] < gap:
            v[a][a // 2] *= -1.0
            v[a + 1][a // 2] *= -1.0
    for i in range(len(v)):
        d = v[i] * scene.cfg.dt
        o[i] = o[i] + (1.0 - be.half_space_move(i, d, 0.5)) * d
    return True


def _rule_while_above(scene, r, be, x, t):  # AnimScripter.cpp:1996-2012, 2019-2030: the component moves in the steps that start with its lowest node above the mark
    moving = bool(x[r["ids"], 1].min() > r["y"])
    if moving == r["moving"]:
        return False
    r["moving"] = moving
    lin, ang, ctr = r["motion"] if moving else (ZERO3, ZERO3, None)
    be.set_dirichlet_motion(0, lin_vel=lin, ang_vel_deg=ang, center=ctr, force_nonzero=True)
    return True


def _rule_let_go(scene, r, be, x, t):
    c = x[r["turn"], r["axis"]]
    if not (c <= r["limit"] if r["below"] else c >= r["limit"]):
        return False
    for g in r["free"]:
        be.end_dirichlet(g, t)
    for g in r["stop"]:
        be.set_dirichlet_motion(g, lin_vel=ZERO3, force_nonzero=True)
    r["done"] = True
    return True


def _rule_pause(scene, r, be, x, t):
    """`script stretchAndPause` (AnimScripter.cpp:1605-1616): the handles move while the turning vertex has not passed x = -0.28;
    from then on every Dirichlet node is held (vertexDBCType ZERO)"""
    if x[r["turn"], 0] >= r["x_limit"]:
        return False
    for g in r["groups"]:
        be.end_dirichlet(g, t)
    for ids in r["ids"]:
        be.add_dirichlet(ids, lin_vel=ZERO3, ang_vel_deg=ZERO3, t0=t, t1=INF)
    r["done"] = True
    return True


def _rule_dragright(scene, r, be, x, t):  # AnimScripter.cpp:1619-1632: let go once the whole body is right of every mesh obstacle
    if x[: r["nSim"], 0].min() > r["x_limit"]:
        be.end_dirichlet(r["group"], t)
        r["done"] = True
        return True
    return False


RULES = {"dco": _rule_dco, "segbed": _rule_segbed, "turn": _rule_turn, "aco": _rule_aco, "while_above": _rule_while_above, "let_go": _rule_let_go,
         "pause": _rule_pause, "dragright": _rule_dragright}  # (the dictionary of `dragright` carries no `kind`)

_families = HANDLE_SCRIPTS + HOLD_SCRIPTS + PULL_SCRIPTS + INITVEL_SCRIPTS + RULE_SCRIPTS + tuple(DCO_SCRIPTS) + CODIM_SCRIPTS
if set(_families) - set(SETUP):
    raise ImportError(f"anim_script.SETUP lacks {sorted(set(_families) - set(SETUP))}")
