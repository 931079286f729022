"""A stand-in for the ctypes binding of librtm3d_hip.so - TEST INFRASTRUCTURE, not a product path.

``record(ir)`` has ``plan.PlanRecorder`` issue a plan on an ``AbiRecorder``, on a machine without the library or a GPU: every
C ABI call is logged by name with its arguments (the context pointer left out), the id out-parameters of tensor and blob
creation are answered with counters, and every call returns 0.  The log is what the runtime would have been told, so its
digest pins the realized launch list of a plan.
"""
import ctypes
import hashlib
import json

from rtm3d_amd import plan as plan_mod

# the plan module's switches as the product sets them (pinned so that RTM3D_* environment variables change nothing)
DEFAULTS = {'V2_MIN_TILES': 200, 'FUSE_LEVEL_ENTRY': True, 'FUSE_LEVEL_TAIL': True, 'FOLD_PROJECT': True, 'FOLD_PROJECT_C128': True,
            'FOLD_NECK_UP': True, 'FUSE_STEM': True, 'USE_CONV128': True, 'USE_CONV64S2': True, 'S2D_ONLY': True, 'BN_TILE_OVERRIDE': {}}


def _value(a):
    """A ctypes argument as plain data (ints, lists, dicts)."""
    if isinstance(a, ctypes.Structure):
        return {name: _value(getattr(a, name)) for name, _ in a._fields_}
    if isinstance(a, ctypes.Array):
        return [_value(v) for v in a]
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if type(a).__name__ == 'CArgObject':          # ctypes.byref(...)
        return _value(a._obj)
    return a


class AbiRecorder(object):
    """The ``rtm3d_*`` entry points of the library, recording."""
    OUT_IDS = {'rtm3d_tensor_create': 'tensor', 'rtm3d_tensor_create_mx8': 'tensor_mx8', 'rtm3d_blob_create': 'blob'}

    def __init__(self):
        self.calls = []
        self._next = {}

    def __getattr__(self, name):
        if not name.startswith('rtm3d_'):
            raise AttributeError(name)

        def call(*args):
            return self._record(name, args)
        return call

    def _record(self, name, args):
        args = args[1:]                                 # (the context pointer)
        if name == 'rtm3d_blob_create':
            data = ctypes.string_at(args[0].value, args[1]) if args[1] else b''
            logged = [int(args[1]), hashlib.sha256(data).hexdigest()]
        elif name in self.OUT_IDS:
            logged = [_value(a) for a in args[:-1]]
        else:
            logged = [_value(a) for a in args]
        if name in self.OUT_IDS:
            kind = self.OUT_IDS[name]
            args[-1]._obj.value = self._next.get(kind, 0)
            self._next[kind] = args[-1]._obj.value + 1
        self.calls.append((name, logged))
        return 0

    def launches(self):
        """The recorded runtime ops (rtm3d_op_*), in order."""
        return [c for c in self.calls if c[0].startswith('rtm3d_op_')]

    def digest(self):
        return hashlib.sha256(json.dumps(self.calls, sort_keys=True).encode()).hexdigest()


def pin_switches(monkeypatch, **switches):
    """Set the plan module's switches to DEFAULTS, but for `switches`."""
    for k, v in dict(DEFAULTS, **switches).items():
        monkeypatch.setattr(plan_mod, k, v)


def record(ir):
    """The AbiRecorder a plan IR was issued on; .recorded is the plan.PlanRecorder that did (op_names, tids ...)."""
    rec = AbiRecorder()
    rec.recorded = plan_mod.PlanRecorder(ir, rec, None)
    return rec
