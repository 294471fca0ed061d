"""TEST INFRASTRUCTURE ONLY -- ctypes loader for ``oracle/c/lqr_oracle.c``."""

import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_NAME = "liblqr_oracle.so"
_lib = None


def _host():
    """The library's stamp: the host CPU (``-march=native``) and the sources it was compiled from."""
    info = open("/proc/cpuinfo").read() if os.path.exists("/proc/cpuinfo") else ""
    cpu = info.split("model name")[1].split("\n")[0] if "model name" in info else ""
    h = hashlib.sha256()
    for name in ("lqr_oracle.c", "lqr_oracle_impl.h"):
        with open(os.path.join(_HERE, "c", name), "rb") as fh:
            h.update(fh.read())
    return f"{cpu}\nsources {h.hexdigest()[:16]}"


def _current(so, host):
    stamp = so + ".host"
    return os.path.exists(so) and os.path.exists(stamp) and open(stamp).read() == host


def _writable(folder):
    try:
        os.makedirs(folder, exist_ok=True)
        probe = os.path.join(folder, f".w{os.getpid()}")
        open(probe, "w").close()
        os.remove(probe)
        return True
    except OSError:
        return False


def _candidates(host):
    """oracle/_build/ first; when the tree is not writable by this user, a per-user cache keyed by the host CPU."""
    key = "lqr_oracle-" + hashlib.sha256(host.encode()).hexdigest()[:12]
    user = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "tfmpc", "oracle", key)
    return [os.path.join(_HERE, "_build"), user, os.path.join(tempfile.gettempdir(), f"tfmpc-oracle-{os.getuid()}", key)]


def build(force=False):
    """Compile the C restatement (gcc, seconds) and return the library's path.  ``-march=native`` is used, so
    the library is rebuilt on a host with another CPU -- into oracle/_build/ when this user may write there,
    else into a per-user cache."""
    host = _host()
    folders = _candidates(host)
    if not force:
        for folder in folders:
            so = os.path.join(folder, _NAME)
            if _current(so, host):
                return so
    for folder in folders:
        if _writable(folder):
            so = os.path.join(folder, _NAME)
            subprocess.check_call(["make", "-s", "-B", "-C", _HERE, f"BUILD={folder}", so])
            with open(so + ".host", "w") as fh:
                fh.write(host)
            return so
    raise RuntimeError("oracle/c_oracle.py: no writable directory for the C restatement: " + ", ".join(folders))


def _load():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def max_threads():
    return int(_load().lqr_oracle_max_threads())


def lqr_solve(F, f, C, c, x0, T, dtype=np.float32, nthreads=1, want_policy=False, want_value=False):
    """Batch LQR solve on the CPU.  ``F[B|1,n,d] f[B|1,n] C[B|1,d,d] c[B|1,d] x0[B,n]``.
    Returns dict with states[B,T+1,n], actions[B,T,m], costs[B,T+1] (+K,k,V,v,const)."""
    lib = _load()
    dt = np.dtype(dtype)
    fn = lib.lqr_oracle_solve_f32 if dt == np.float32 else lib.lqr_oracle_solve_f64
    x0 = np.ascontiguousarray(x0, dtype=dt)
    B, n = x0.shape
    arrs, strides = [], []
    for a, tail in ((F, 2), (f, 1), (C, 2), (c, 1)):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.ndim == tail:
            a = a[None]
        assert a.shape[0] in (1, B)
        arrs.append(a)
        strides.append(0 if a.shape[0] == 1 and B > 1 else int(np.prod(a.shape[1:])))
    F, f, C, c = arrs
    d = F.shape[-1]
    m = d - n
    out = dict(states=np.empty((B, T + 1, n), dt), actions=np.empty((B, T, m), dt),
               costs=np.empty((B, T + 1), dt))
    if want_policy:
        out.update(K=np.empty((B, T, m, n), dt), k=np.empty((B, T, m), dt))
    if want_value:
        out.update(V=np.empty((B, T, n, n), dt), v=np.empty((B, T, n), dt), const=np.empty((B, T), dt))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    L = ctypes.c_long
    rc = fn(ctypes.c_int(B), ctypes.c_int(n), ctypes.c_int(m), ctypes.c_int(T),
            p(F), L(strides[0]), p(f), L(strides[1]), p(C), L(strides[2]), p(c), L(strides[3]),
            p(x0), p(out["states"]), p(out["actions"]), p(out["costs"]),
            p(out.get("K")), p(out.get("k")), p(out.get("V")), p(out.get("v")), p(out.get("const")),
            ctypes.c_int(nthreads))
    out["status"] = int(rc)
    return out
