"""An exact, comparable picture of what ipc_amd/scene_script.py makes of a scene: `dump(sc)` of an AssembledScene, `dump_apply(sc)` of the backend calls of
apply(), and `Recorder`, the backend that notes them.  Everything is stored so that equality means "the same to the last bit": a float as its float.hex(),
a small array element by element, a large one as the SHA-256 of its bytes.  tools/make_scene_assembly_golden.py writes tests/golden/scene_assembly.json with
it (the `digest` of each dump; the tool prints the dump itself), tests/test_scene_assembly_golden.py compares against that file.  No GPU, nothing of the reference."""
import dataclasses
import hashlib
import json

import numpy as np

from ipc_amd import scene_script as ss

INLINE = 64  # arrays of at most this many elements are stored element by element
SKIP = ("cfg", "read_seq")  # the input itself, and a callable


def _scalar(x):
    if isinstance(x, float):
        return x.hex()  # ("inf", "-inf" and "nan" included)
    if isinstance(x, str):
        return "s:" + x  # (no float.hex() starts like this)
    return x  # None, bool, int


def _array(a):
    a = np.asarray(a)
    out = {"dtype": a.dtype.str, "shape": list(a.shape)}
    if a.size <= INLINE:
        out["data"] = [_scalar(v) for v in a.ravel().tolist()]
    else:
        out["sha256"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


def _walk(x, name, out):
    """leaves of x in order under names that spell the containers: `[i]` a list, `(i)` a tuple, `.key` a dict"""
    if isinstance(x, dict):
        for k, v in x.items():
            _walk(v, f"{name}.{k}", out)
        if not x:
            out[name] = "empty dict"
    elif isinstance(x, (list, tuple)):
        a, b = "[]" if isinstance(x, list) else "()"
        for i, v in enumerate(x):
            _walk(v, f"{name}{a}{i}{b}", out)
        if not x:
            out[name] = "empty list" if isinstance(x, list) else "empty tuple"
    elif isinstance(x, (np.ndarray, np.generic)):  # (a numpy scalar: a 0-d array, so that it differs from the Python number)
        out[name] = _array(x)
    elif x is None or isinstance(x, (bool, int, float, str)):
        out[name] = _scalar(x)
    else:
        raise TypeError(f"{name}: {type(x).__name__} has no exact form here")


def dump(x, name=""):
    """flat, ordered {name: value}: of an AssembledScene every field but `cfg` and `read_seq`, of anything else its leaves"""
    out = {}
    if dataclasses.is_dataclass(x):
        for f in dataclasses.fields(x):
            if f.name not in SKIP:
                _walk(getattr(x, f.name), f.name, out)
    else:
        _walk(x, name, out)
    return out


def digest(x):
    """SHA-256 of a dump (or a list of calls, or of steps) in its one JSON spelling, the order of the names included: equal digests, equal to the last bit"""
    return hashlib.sha256(json.dumps(x, separators=(",", ":")).encode()).hexdigest()


class Recorder:
    """A backend that does nothing but note its calls: `calls` is a list of [method name, dump of (args, kwargs)].  It answers what apply() and before_step()
    read: the index of a new half-space, 1.0 (the whole move admitted) from half_space_move, and a state() with the positions `V` the caller sets."""

    def __init__(self, V=None):
        self.calls = []
        self.V = V
        self._planes = 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def method(*args, **kwargs):
            self.calls.append([name, dump({"a": list(args), "k": kwargs})])
            if name == "add_half_space":
                self._planes += 1
                return self._planes - 1
            if name == "half_space_move":
                return 1.0
            if name == "state":
                return {"V": self.V}
            return None
        return method


def dump_apply(sc):
    be = Recorder()
    ss.apply(sc, be)
    return be.calls
