"""A recording stand-in for libloamlivox_hip.so, for the CPU tier of loam_livox_amd/api.py (tests/test_api_handles_host.py,
tests/test_api_calls_host.py): every ll_* attribute is a function that logs its name and its arguments and answers 0.  No device and no
shared library are needed; install it with monkeypatch.setattr(capi, "_lib", Recording_library()).

An argument is logged as its scalar value; as dtype, shape and content of a numpy array (ptr() keeps the array on the pointer it makes);
as the value of a handle or raw pointer; as the element type and content of a ctypes array; or as {"byref": type, "value": ...} with the
value the callee finds there.  A byref(c_void_p) receives a fresh non-null value, so that ll_*_create yields a handle.  `fail` names the
functions that answer -1, `answer()` sets a function's return value and what it writes through its byref arguments."""
import ctypes as C
import hashlib

import numpy as np

_CArg = type(C.byref(C.c_int32(0)))


def plain(v):
    """a value as JSON can hold it: what a call was given, or what a method returned"""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, np.generic):
        return plain(v.item())
    if isinstance(v, np.ndarray):
        raw = np.ascontiguousarray(v).tobytes()
        return {"dtype": str(v.dtype), "shape": list(v.shape), "bytes": raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()[:24]}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, C.Structure):
        return {"struct": type(v).__name__, "bytes": bytes(v).hex()}
    if isinstance(v, C.Array):
        return {"array": v._type_.__name__, "values": [plain(x) for x in v]}
    if isinstance(v, C.c_void_p):
        arr = getattr(v, "_arr", None)   # numpy's data_as() leaves the array here
        return plain(arr) if arr is not None else {"pointer": v.value}
    if isinstance(v, C._SimpleCData):
        return {"ctype": type(v).__name__, "value": plain(v.value)}
    if isinstance(v, _CArg):
        o = v._obj
        return {"byref": type(o).__name__, "value": plain(o) if isinstance(o, C.Structure) else plain(o.value)}
    return {"object": type(v).__name__}


class Recording_library:
    def __init__(self):
        self.calls = []        # [name, [arguments]] in call order
        self.fail = set()      # these answer -1
        self._answers = {}
        self._next_handle = 0x1000

    def answer(self, name: str, ret=0, out=None):
        """`name` returns ret and writes out[i] through its i-th argument (a byref)"""
        self._answers[name] = (ret, dict(out or {}))

    def names(self):
        return [c[0] for c in self.calls]

    def of(self, name: str):
        """the argument lists of the calls of one function"""
        return [c[1] for c in self.calls if c[0] == name]

    def __getattr__(self, name):
        if not name.startswith("ll_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append([name, [plain(a) for a in args]])
            if name == "ll_last_error":
                return b"the stand-in was told to fail"
            if name in self.fail:
                return -1
            ret, out = self._answers.get(name, (0, {}))
            for i, a in enumerate(args):
                if i in out:
                    a._obj.value = out[i]
                elif isinstance(a, _CArg) and isinstance(a._obj, C.c_void_p):
                    a._obj.value = self._next_handle
                    self._next_handle += 0x10
            return ret
        fn.__name__ = name
        setattr(self, name, fn)
        return fn
