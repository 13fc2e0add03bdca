"""CPU: per-model option sets -- admmnet_options_intern / admmnet_options_describe and the handle in admmnet_cfg through the built
library (it loads without a GPU), ``admm_net_amd.Options`` and ``model.options``, and the interning table of csrc/options.h under
the address, undefined-behaviour and thread sanitizers in a stand-alone program (tests/host_model/options_model.cpp).
The environment route is the yardstick throughout: an option set must resolve to what the same variables give in the environment
(tests/host_model/route_model) and carve the workspace sizes recorded for them (tests/route_workspace_sizes.json)."""
import copy
import ctypes
import json
import os
import pickle
import subprocess
import sys

import pytest

import admm_net_amd as A
from admm_net_amd import _lib
from admm_net_amd.options import describe
from test_route_host import BATCHES, ENVS, GEOMS, SIZES, clean_env

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host_model")
# every environment of the route tests as an option set (ADMMNET_TEST_CHUNK is the tests' own variable: model.chunk)
SETS = {name: {k: v for k, v in env.items() if k != "ADMMNET_TEST_CHUNK"} for name, env in ENVS.items()}


def kwargs(env):
    return {k[len("ADMMNET_"):].lower(): v for k, v in env.items()}


def intern(pairs):
    """admmnet_options_intern on a list of (name, value); None passes a NULL pointer."""
    lib = _lib.load()
    n = len(pairs)
    enc = [[None if s is None else s.encode() for s in col] for col in zip(*pairs)] if n else [[], []]
    h = lib.admmnet_options_intern((ctypes.c_char_p * n)(*enc[0]), (ctypes.c_char_p * n)(*enc[1]), n)
    if h < 0:
        _lib.check(h, "admmnet_options_intern")
    return h


def run_child(code, env, *args):
    p = subprocess.run([sys.executable, "-c", code, *args], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


# ---- 1. interning -------------------------------------------------------------------------------------------------------------------
def test_same_settings_same_handle():
    a = intern([("ADMMNET_SPECTRAL_ITERS", "41"), ("ADMMNET_EIG", "ql"), ("ADMMNET_ARROW", "0")])
    assert a >= 1
    assert intern([("ADMMNET_ARROW", "0"), ("ADMMNET_EIG", "ql"), ("ADMMNET_SPECTRAL_ITERS", "41")]) == a      # order
    assert intern([("ADMMNET_ARROW", "00"), ("ADMMNET_EIG", "ql"), ("ADMMNET_SPECTRAL_ITERS", "041")]) == a    # spelling
    assert intern([("ADMMNET_ARROW", "0 "), ("ADMMNET_EIG", "ql"), ("ADMMNET_SPECTRAL_ITERS", " 41")]) == a
    b = intern([("ADMMNET_ARROW", "0"), ("ADMMNET_EIG", "ql"), ("ADMMNET_SPECTRAL_ITERS", "42")])
    assert b >= 1 and b != a
    assert intern([("ADMMNET_SPECTRAL_ITERS", "41"), ("ADMMNET_EIG", "ql"), ("ADMMNET_ARROW", "0")]) == a      # and it stays
    assert A.Options(arrow=0, eig="ql", spectral_iters=41).handle == a
    assert A.Options(spectral_iters="041", eig="ql", arrow=False).handle == a


def test_defaults_are_handle_zero():
    assert intern([]) == 0
    base = describe(0)
    assert intern([("ADMMNET_SPECTRAL", str(base["spectral"])), ("ADMMNET_SPECTRAL_ITERS", str(base["spectral_iters"])),
                   ("ADMMNET_SPECTRAL_TOL", repr(base["spectral_tol"]))]) == 0
    assert A.Options().handle == 0 and A.Options(lean=None, eig=None).handle == 0
    assert A.Options(spectral=base["spectral"]).handle == 0


def test_errors_name_the_offender():
    with pytest.raises(_lib.AdmmNetError, match="ADMMNET_NO_SUCH_SWITCH"):
        intern([("ADMMNET_SPECTRAL", "0"), ("ADMMNET_NO_SUCH_SWITCH", "1")])
    with pytest.raises(_lib.AdmmNetError, match="ADMMNET_NO_SUCH_SWITCH"):
        A.Options(no_such_switch=1).handle
    with pytest.raises(_lib.AdmmNetError, match="ADMMNET_TEST_CHUNK"):   # the tests' own variable is no switch of the library
        A.Options(test_chunk=1).handle
    with pytest.raises(_lib.AdmmNetError, match="value 1 is NULL for ADMMNET_EIG"):
        intern([("ADMMNET_SPECTRAL", "0"), ("ADMMNET_EIG", None)])
    with pytest.raises(_lib.AdmmNetError, match="name 0 is NULL"):
        intern([(None, "0"), ("ADMMNET_EIG", "ql")])
    lib = _lib.load()
    assert lib.admmnet_options_intern(None, None, 2) == -1 and b"NULL" in lib.admmnet_last_error()


@pytest.mark.parametrize("handle", [4097, 1 << 20, -1])
def test_a_handle_never_issued_is_refused(handle):
    """4096 sets fit the table and this process interns a handful: none of these was issued.  Every entry point that takes a
    cfg refuses it as an argument error, before it touches the device."""
    lib = _lib.load()
    m = A.PhiEstADMMNet(M=4, N=4, num_layers=3)
    cfg = m.cfg()
    cfg.reserved[1] = handle
    ref = ctypes.byref(cfg)
    assert lib.admmnet_workspace_bytes(ref, 4) == -1 and lib.admmnet_glayer_workspace_bytes(ref, 4) == -1
    with pytest.raises(_lib.AdmmNetError, match=r"reserved\[0\] = %d " % handle):
        _lib.check(-1, "admmnet_workspace_bytes")
    one = ctypes.c_void_p(256)   # (never dereferenced: the argument check comes first)
    calls = {
        "admmnet_begin": lambda: lib.admmnet_begin(ref, 4, one, 1 << 40, None, None),
        "admmnet_forward_f32": lambda: lib.admmnet_forward_f32(ref, one, one, one, one, 4, one, None, one, 1 << 40, None, None),
        "admmnet_layer_front": lambda: lib.admmnet_layer_front(ref, one, 0, one, one, one, 4, one, None, None, None),
        "admmnet_layer_back": lambda: lib.admmnet_layer_back(ref, one, 0, 4, one, one, None),
        "admmnet_layer_back_pair": lambda: lib.admmnet_layer_back_pair(ref, one, 0, 4, one, one, None),
        "admmnet_finish": lambda: lib.admmnet_finish(ref, one, 4, one, one, None, None),
        "admmnet_glayer_f32": lambda: lib.admmnet_glayer_f32(ref, one, one, one, None, 4, one, None, None, one, 1 << 40, None, None),
        "admmnet_glayer_spectral_f32": lambda: lib.admmnet_glayer_spectral_f32(ref, one, one, one, one, 0, None, None, None, None, 4,
                                                                               one, one, one, one, 0, None),
        "admmnet_eigh_c64_o": lambda: lib.admmnet_eigh_c64_o(17, 4, one, one, one, one, 1 << 40, None, None, handle),
    }
    for name, call in calls.items():
        assert call() == -1, name
        with pytest.raises(_lib.AdmmNetError, match=str(handle)):
            _lib.check(-1, name)
    assert lib.admmnet_eigh_workspace_bytes_o(17, 4, handle) == -1
    buf = ctypes.create_string_buffer(64)
    assert lib.admmnet_options_describe(handle, buf, 64) == -1 and str(handle).encode() in lib.admmnet_last_error()
    with pytest.raises(_lib.AdmmNetError, match=str(handle)):
        describe(handle)


DESCRIBE_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.admmnet_options_intern.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32]
lib.admmnet_options_describe.restype, lib.admmnet_options_describe.argtypes = ctypes.c_int64, [ctypes.c_int32, ctypes.c_char_p, ctypes.c_int64]
out = {}
for name, env in json.loads(sys.argv[2]).items():
    n = len(env)
    h = lib.admmnet_options_intern((ctypes.c_char_p * n)(*[k.encode() for k in env]), (ctypes.c_char_p * n)(*[v.encode() for v in env.values()]), n)
    buf = ctypes.create_string_buffer(4096)
    length = lib.admmnet_options_describe(h, buf, 4096)
    assert length == len(buf.value), (length, len(buf.value))
    out[name] = [h, buf.value.decode()]
print("RESULT " + json.dumps(out))
"""


def test_describe_is_what_the_environment_resolves_to(tmp_path):
    """In one process with a clean environment every set of the route tests is interned and described; the text must be, line
    for line, what tests/host_model/route_model prints for the same variables set in ITS environment: one parser, two sources."""
    exe = str(tmp_path / "route_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(HOST, "route_model.cpp"), "-o", exe])
    got = run_child(DESCRIBE_CHILD, clean_env({}), _lib.LIB_PATH, json.dumps(SETS))
    handles = {}
    for name, env in SETS.items():
        want = subprocess.run([exe, "switches"], env=clean_env(env), capture_output=True, text=True, check=True).stdout
        assert got[name][1] == want, name
        handles.setdefault(want, set()).add(got[name][0])
    assert got["default"][0] == 0
    assert all(len(h) == 1 for h in handles.values())                     # equal settings, equal handle
    assert len({next(iter(h)) for h in handles.values()}) == len(handles)   # different settings, different handle


# ---- 2. precedence: built-in < environment < options ------------------------------------------------------------------------------
PRECEDENCE_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import admm_net_amd as A
from admm_net_amd.options import describe
out = {"defaults": describe(0), "arrow": A.Options(arrow=0).resolved(), "back_on": A.Options(spectral=1).resolved(),
       "handles": [A.Options().handle, A.Options(spectral=0).handle, A.Options(arrow=0).handle, A.Options(spectral=1).handle]}
print("RESULT " + json.dumps(out))
"""


def test_options_override_the_environment_which_overrides_the_built_in_values():
    got = run_child(PRECEDENCE_CHILD, clean_env({"ADMMNET_SPECTRAL": "0", "ADMMNET_SPECTRAL_ITERS": "7"}), ROOT)
    assert got["defaults"]["spectral"] == 0 and got["defaults"]["spectral_iters"] == 7 and got["defaults"]["arrow"] == 1
    assert got["arrow"]["spectral"] == 0 and got["arrow"]["arrow"] == 0 and got["arrow"]["spectral_iters"] == 7
    assert got["back_on"]["spectral"] == 1 and got["back_on"]["arrow"] == 1 and got["back_on"]["spectral_iters"] == 7
    h = got["handles"]
    assert h[0] == 0 and h[1] == 0 and h[2] >= 1 and h[3] >= 1 and h[2] != h[3]   # (spectral=0 restates this environment)


# ---- 3. workspace sizes ----------------------------------------------------------------------------------------------------------------
SIZES_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
class Cfg(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("M", "N", "L", "K", "has_head", "chunk", "sub_batch", "reserved")]
lib.admmnet_options_intern.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32]
for f in (lib.admmnet_workspace_bytes, lib.admmnet_glayer_workspace_bytes):
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.POINTER(Cfg), ctypes.c_int64]
lib.admmnet_eigh_workspace_bytes_o.restype = ctypes.c_int64
lib.admmnet_eigh_workspace_bytes_o.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]
sets = json.loads(sys.argv[2])
handles = {}
for name, env in sets.items():   # all interned first: every size below is asked with the other sets in the table
    n = len(env)
    handles[name] = lib.admmnet_options_intern((ctypes.c_char_p * n)(*[k.encode() for k in env]),
                                               (ctypes.c_char_p * n)(*[v.encode() for v in env.values()]), n)
    assert handles[name] >= 0, name
out = {}
for name in sets:
    h = handles[name]
    rows = []
    for M, N in json.loads(sys.argv[3]):
        for B, chunk, sub in json.loads(sys.argv[4]):
            cfg = Cfg(M, N, 3, 3, 0, chunk, sub, h)
            rows.append([lib.admmnet_workspace_bytes(ctypes.byref(cfg), B), lib.admmnet_glayer_workspace_bytes(ctypes.byref(cfg), B),
                         lib.admmnet_eigh_workspace_bytes_o(M * N + 1, B, h)])
    out[name] = rows
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def option_sizes():
    return run_child(SIZES_CHILD, clean_env({}), _lib.LIB_PATH, json.dumps(SETS), json.dumps(GEOMS), json.dumps(BATCHES))


@pytest.mark.parametrize("name", list(SETS))
def test_workspace_sizes_equal_the_environment_route(option_sizes, name):
    """One process, clean environment, every set interned side by side: admmnet_workspace_bytes, admmnet_glayer_workspace_bytes
    and admmnet_eigh_workspace_bytes_o under the handle answer what the record holds the environment route to."""
    with open(SIZES) as fh:
        want = json.load(fh)[name]
    assert option_sizes[name] == want


# ---- 4. the module -------------------------------------------------------------------------------------------------------------------
def test_options_value():
    o = A.Options(spectral=0, eig="ql", spectral_tol=3e-7, lean=None)
    assert o.overrides == {"eig": "ql", "spectral": "0", "spectral_tol": "3e-07"}
    assert repr(o) == "Options(eig='ql', spectral='0', spectral_tol='3e-07')"
    assert o == A.Options(spectral_tol="3.0e-7", spectral="00", eig="ql") and hash(o) == hash(A.Options(spectral_tol="3.0e-7", spectral="00", eig="ql"))
    assert o != A.Options(spectral=0, eig="ql") and o != "Options" and A.Options() == A.Options(spectral_iters=describe(0)["spectral_iters"])
    assert len({o, A.Options(eig="ql", spectral=False, spectral_tol=3e-7), A.Options()}) == 2
    r = o.resolved()
    assert r["spectral"] == 0 and r["eig"] == 1 and abs(r["spectral_tol"] - 3e-7) < 1e-13 and set(r) == set(describe(0))
    with pytest.raises(AttributeError):
        o.spectral = 1
    with pytest.raises(AttributeError):
        o._overrides = ()
    with pytest.raises(ValueError):
        A.Options(**{"ADMMNET_SPECTRAL": 0})
    assert A.Options(spectral=True).overrides == {"spectral": "1"}   # (str(True) would read as 0)


def test_model_options():
    import torch
    m = A.ADMMNet(M=4, N=4, num_layers=3)
    assert m.options is None and m.cfg().reserved[1] == 0
    keys = set(m.state_dict())
    o = A.Options(spectral=0, spectral_iters=43)
    m.sub_batch = 5
    m._ws = torch.empty(8, dtype=torch.uint8)
    m.options = o
    assert m._ws is None                                              # (the carve depends on the route)
    assert m.options is o and m.cfg().reserved[1] == o.handle >= 1 and m.cfg().reserved[0] == 5
    assert set(m.state_dict()) == keys and not any("option" in k for k in keys)
    other = A.ADMMNet(M=4, N=4, num_layers=3)
    other.load_state_dict(m.state_dict())
    assert other.options is None and other.cfg().reserved[1] == 0     # not part of the state_dict
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert clone.options == o and clone.options is not o and clone.cfg().reserved[1] == o.handle and clone.sub_batch == 5
    m._ws = torch.empty(8, dtype=torch.uint8)
    m.options = None
    assert m._ws is None and m.cfg().reserved[1] == 0
    with pytest.raises(TypeError):
        m.options = {"spectral": 0}
    # the handle reaches the carve: the size under the option set is the size recorded for its environment
    lib = _lib.load()
    with open(SIZES) as fh:
        rec = json.load(fh)
    i = GEOMS.index((2, 4)) * len(BATCHES)
    m8 = A.PhiEstADMMNet(M=2, N=4, num_layers=3)
    for name in ("default", "spectral_unfused", "eig_ql"):
        m8.options = A.Options(**kwargs(SETS[name]))
        assert lib.admmnet_workspace_bytes(ctypes.byref(m8.cfg()), BATCHES[0][0]) == rec[name][i][0], name


UNPICKLE_CHILD = r"""
import json, pickle, sys
sys.path.insert(0, sys.argv[1])
import admm_net_amd as A
first = A.Options(dc_occ=6, pn_split=8).handle          # this process's table starts differently
o, m = pickle.loads(bytes.fromhex(sys.argv[2]))
print("RESULT " + json.dumps({"first": first, "handle": o.handle, "resolved": o.resolved(), "model": m.options.resolved(),
                               "cfg": m.cfg().reserved[1], "repr": repr(o), "defaults": A.options.describe(0)}))
"""


def test_a_pickled_options_interns_again_where_it_lands():
    o = A.Options(eig="ql", spectral=0, spectral_tol=3e-7)
    m = A.PhiEstADMMNet(M=4, N=4, num_layers=3)
    m.options = o
    assert o.handle >= 1
    blob = pickle.dumps((o, m))
    got = run_child(UNPICKLE_CHILD, clean_env({}), ROOT, blob.hex())
    assert got["first"] == 1 and got["handle"] == 2 and got["cfg"] == 2
    # (this process may run under ADMMNET_* variables of its own; the child's environment is clean: compare what the set names)
    assert got["repr"] == repr(o) and got["resolved"] == got["model"]
    assert (got["resolved"]["eig"], got["resolved"]["spectral"]) == (1, 0) and abs(got["resolved"]["spectral_tol"] - 3e-7) < 1e-13
    assert {k: v for k, v in got["resolved"].items() if k not in ("eig", "spectral", "spectral_tol")} == \
           {k: v for k, v in got["defaults"].items() if k not in ("eig", "spectral", "spectral_tol")}


# ---- 5. the table under the sanitizers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_table_under_sanitizers(tmp_path, sanitizer):
    """tests/host_model/options_model.cpp (its own main, csrc/options.h only): eight threads intern overlapping sets while four
    resolve, one handle per distinct set; unknown names and NULL pointers; the table filled to its 4096 entries refuses the next
    set and writes nothing past the end."""
    exe = str(tmp_path / "options_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "options_model.cpp"), "-o", exe])
    p = subprocess.run([exe], env=clean_env({}), capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "ok"
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]


def test_training_route_solves_under_the_model_options(monkeypatch):
    """training.unrolled_forward's default solver is ops.eigh under ``model.options`` (so Options(eig="ql") reaches the training
    route's eigensolver); a solver handed in is used as given.  ops.eigh is replaced by a CPU stand-in that records its call."""
    import torch
    from admm_net_amd import ops, training
    seen = []

    def eigh(A_, options=None):
        seen.append(options)
        return torch.linalg.eigh(A_)

    monkeypatch.setattr(ops, "eigh", eigh)
    torch.manual_seed(0)
    m = A.PhiEstADMMNet(M=2, N=3, num_layers=3)
    y, b = (torch.randn(2, 6, dtype=torch.complex64) for _ in range(2))
    sigma = torch.full((2,), 0.1)
    o = A.Options(eig="ql", spectral=0)
    m.options = o
    phi = training.unrolled_forward(m, y, b, sigma, assembler=training.TorchAssembler)
    assert len(seen) == 2 and all(s is o for s in seen)   # (the G-layers k = 0 .. K - 2)
    m.options = None
    del seen[:]
    phi0 = training.unrolled_forward(m, y, b, sigma, assembler=training.TorchAssembler)
    assert seen == [None, None] and torch.equal(phi0, phi)
    del seen[:]
    training.unrolled_forward(m, y, b, sigma, solver=torch.linalg.eigh, assembler=training.TorchAssembler)
    assert seen == []
