"""CPU: csrc/route.h -- the one reader of the ADMMNET_* switches and the one derivation of the kernel route -- through
tests/host_model/route_model.cpp (plain g++), and the workspace sizes the carve gives through the built library.
The expected values are written out here from the code before route.h existed (the "parent"): the getenv expressions that
were spread over the launchers, and the route their nested decisions gave."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_variants import VARIANTS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
SIZES = os.path.join(ROOT, "tests", "route_workspace_sizes.json")

# every environment the route and workspace tests run under (a new entry of VARIANTS joins by itself)
ENVS = dict({"default": {}}, **VARIANTS)
ENVS.update({"streams_2": {"ADMMNET_STREAMS": "2"}, "pad_min_150": {"ADMMNET_PAD_MIN": "150"}, "pad_min_999": {"ADMMNET_PAD_MIN": "999"}})


def clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ADMMNET_")}
    env.update({k: v for k, v in extra.items() if v is not None})
    return env


@pytest.fixture(scope="module")
def model():
    exe = os.path.join(ROOT, "tests", "host_model", "route_model")
    src = exe + ".cpp"
    hdr = os.path.join(CSRC, "route.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, src, "-o", exe])

    def run(args, env, text=True):
        return subprocess.run([exe] + args, env=clean_env(env), capture_output=True, text=text, check=True).stdout
    return run


# ---- 1. parsing ---------------------------------------------------------------------------------------------------------------
RAW = [None, "", "0", "1", "00", "off", "2"]                      # None = unset; each switch adds its own keyword
UNSET = -1000                                                     # what the model prints for an unset ADMMNET_PAD_MIN


def _on(e): return int(not (e is not None and _atoi(e) == 0))      # !(getenv(X) && atoi(getenv(X)) == 0)
def _word(w): return lambda e: int(e == w)                         # getenv(X) && !strcmp(getenv(X), w)
def _present(e): return int(e is not None)                         # getenv(X) != nullptr
def _int(unset): return lambda e: unset if e is None else _atoi(e)   # getenv(X) ? atoi(getenv(X)) : unset


def _atoi(e):
    m = re.match(r"\s*[+-]?\d+", e)
    return int(m.group(0)) if m else 0


PARSE = {   # switch: (its own keyword, the parent's expression as a function of the raw string)
    "ADMMNET_SPECTRAL": ("0", _on), "ADMMNET_SPECTRAL_FUSED": ("0", _on), "ADMMNET_SF_FOLD": ("0", _on),
    "ADMMNET_SF_SMALLWG": ("0", _on), "ADMMNET_ARROW": ("0", _on), "ADMMNET_ARROW_FUSED": ("0", _on),
    "ADMMNET_LEAN": ("0", _on), "ADMMNET_FUSE_BACK": ("0", _on),
    "ADMMNET_EIG": ("ql", _word("ql")), "ADMMNET_TRIDIAG": ("lds", _word("lds")), "ADMMNET_TRIDIAG_BIG": ("sweep", _word("sweep")),
    "ADMMNET_BACK": ("q", _word("q")), "ADMMNET_REBUILD": ("tiles", _word("tiles")),
    "ADMMNET_DC_BLOCKS": ("0", lambda e: int(e != "0")),
    "ADMMNET_PN_SPLIT": ("8", lambda e: 0 if e == "0" else 8 if e == "8" else 84),
    "ADMMNET_STREAMS": ("2", lambda e: int(e is not None and _atoi(e) == 2)),
    "ADMMNET_TR_OCC": ("2", lambda e: int(not (e is not None and _atoi(e) == 2))),
    "ADMMNET_SF_TIMING": ("1", _present), "ADMMNET_AR_TIMING": ("1", _present), "ADMMNET_BR_TIMING": ("1", _present),
    "ADMMNET_PN_TIMING": ("1", _present), "ADMMNET_DC_TIMING": ("1", _present), "ADMMNET_DC_POISON": ("1", _present),
    "ADMMNET_PAD_MIN": ("150", _int(UNSET)), "ADMMNET_DC_OCC": ("6", _int(0)), "ADMMNET_TR_PAD_LDS": ("100000", _int(0)),
    "ADMMNET_SPECTRAL_ITERS": ("3", _int(5)),
    "ADMMNET_SPECTRAL_TOL": ("3e-7", lambda e: np.float32(1e-6) if e is None else np.float32(float(e)) if re.match(r"[\d.]", e) else np.float32(0)),
}


def read_switches(model, env):
    return dict(ln.split() for ln in model(["switches"], env).splitlines())


@pytest.mark.parametrize("name", sorted(PARSE))
def test_switch_parsing_matches_the_parent_expressions(model, name):
    """Each switch keeps the spellings its own getenv expression accepted in the parent:
      !(getenv(X) && atoi(getenv(X)) == 0)        SPECTRAL, SPECTRAL_FUSED, SF_FOLD, SF_SMALLWG, ARROW, ARROW_FUSED, LEAN, FUSE_BACK
      getenv(X) && !strcmp(getenv(X), "word")     EIG ql, TRIDIAG lds, TRIDIAG_BIG sweep, BACK q, REBUILD tiles
      !(getenv(X) && !strcmp(getenv(X), "0"))     DC_BLOCKS
      (e && !strcmp(e, "0")) ? 0 : (e && !strcmp(e, "8")) ? 8 : 84     PN_SPLIT
      getenv(X) && atoi(getenv(X)) == 2           STREAMS;  !(... == 2) TR_OCC
      getenv(X) != nullptr                        SF_TIMING, AR_TIMING, BR_TIMING, PN_TIMING, DC_TIMING, DC_POISON
      getenv(X) ? atoi(getenv(X)) : d             PAD_MIN (d = 129 / 176 by SPECTRAL, in route_for), DC_OCC 0, TR_PAD_LDS 0, SPECTRAL_ITERS 5
      getenv(X) ? (float)atof(getenv(X)) : 1e-6f  SPECTRAL_TOL
    and setting one switch moves no other."""
    keyword, expr = PARSE[name]
    base = read_switches(model, {})
    assert set(base) == set(PARSE)
    for raw in RAW + [keyword]:
        got = read_switches(model, {name: raw})
        want = expr(raw)
        if name == "ADMMNET_SPECTRAL_TOL":
            assert np.float32(float(got[name])) == want, (raw, got[name])
        else:
            assert int(got[name]) == want, (raw, got[name])
        assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in base.items() if k != name}, raw


# ---- 2. routes at the edges -----------------------------------------------------------------------------------------------------
EDGES = [1, 7, 8, 96, 97, 112, 113, 128, 129, 130, 160, 175, 176, 192, 255, 256]
BUFS = {1: "Wdc", 2: "log", 4: "panel", 8: "spec_mat", 16: "spec_flag"}


def read_routes(model, env, Ds):
    return [dict(kv.split("=") for kv in ln.split()) for ln in model(["routes"] + [str(d) for d in Ds], env).splitlines()]


def row(r):
    """One route as a line of the tables below: eigen dimension (D = the geometry's own) | state storage | first layer |
    tridiagonalisation (+Q: explicit Q) | tridiagonal solver | back-transform | rebuild | matrix function | buffers | error."""
    first = r["first"] + ("+" + r["first_rebuild"] if r["first"] == "AR_GLOBAL" else "")
    solver = ("dc" if r["dc"] == "1" else "ql") + ("/rowmajor" if r["rowmajor"] == "1" else "") + ("/colmap" if r["colmap"] == "1" else "")
    mf = r["matfun"] + ("+late" if r["late_image"] == "1" else "") + ("+fold" if r["fold"] == "1" else "")
    bufs = "+".join(v for b, v in BUFS.items() if int(r["buffers"]) & b)
    return " ".join(["D" if r["eig_dim"] == r["D"] else r["eig_dim"], r["storage"], first, r["tridiag"] + ("+Q" if r["explicit_q"] == "1" else ""),
                     solver, r["back"], r["rebuild"], mf, bufs, r["error"]])


# The routes the parent took, by reading its carve_chunk / use_lean / eig_dim / admmnet_layer_front / eig_chunk and the launchers
# behind them.  Per environment: (first D, last D, row).
SMALL = "D lean AR_LDS reg+Q dc in_rebuild back_rebuild %s Wdc%s none"          # D <= 128 on the default pipeline
PADDED = "256 half AR_FUSED panel dc/colmap wy_apply rebuild_big %s Wdc+panel%s none"
E_SMALL, E_PAD = SMALL % ("off", ""), PADDED % ("off", "")
E_SWEEP = "D full AR_FUSED sweep+Q dc vgemm_big rebuild off Wdc none"           # 128 < D < 256 at its own size
E_256 = E_PAD.replace("256 half", "D half")
EIGEN_ONLY = [(1, 128, E_SMALL), (129, 175, E_SWEEP), (176, 255, E_PAD), (256, 256, E_256)]


def spectral(mf_small, mf_big, bufs="+spec_flag"):
    small, big = SMALL % (mf_small, bufs), PADDED % (mf_big, bufs)
    return [(1, 7, SMALL % ("off", bufs)), (8, 128, small), (129, 255, big), (256, 256, big.replace("256 half", "D half"))]


DEFAULT = spectral("fused+fold", "fused+late+fold")
EXPECTED = {
    "default": DEFAULT,
    "eigen_only": EIGEN_ONLY,
    "eig_ql": [(1, 128, "D lean AR_LDS reg+Q ql rotation rebuild off log none"),
               (129, 255, "D full AR_FUSED sweep+Q ql rotation rebuild off log none"),
               (256, 256, "D full AR_FUSED panel+Q ql rotation rebuild_big off log none")],
    "no_arrow": [(1, 128, "D full dense reg+Q dc in_rebuild back_rebuild off Wdc none"),
                 (129, 175, E_SWEEP.replace("AR_FUSED", "dense")),
                 (176, 255, E_PAD.replace("half AR_FUSED", "full dense")),
                 (256, 256, E_256.replace("half AR_FUSED", "full dense"))],
    "unfused_back": [(1, 128, "D full dense reg+Q dc/rowmajor vgemm rebuild off Wdc none"),
                     (129, 175, E_SWEEP.replace("AR_FUSED", "dense")),
                     (176, 255, E_PAD.replace("half AR_FUSED", "full dense")),
                     (256, 256, E_256.replace("half AR_FUSED", "full dense"))],
    "tridiag_lds": [(1, 128, "D full dense lds+Q dc in_rebuild back_rebuild off Wdc none"),
                    (129, 255, "D full dense lds+Q dc vgemm_big rebuild off Wdc none"),
                    (256, 256, "D full dense lds+Q dc vgemm_big rebuild_big off Wdc+panel none")],
    "full_storage": [(1, 128, E_SMALL.replace("lean", "full")), (129, 175, E_SWEEP),
                     (176, 255, E_PAD.replace("half", "full")), (256, 256, E_256.replace("half", "full"))],
    "sweep_big": [(1, 128, E_SMALL), (129, 255, E_SWEEP),
                  (256, 256, "D full AR_FUSED sweep+Q dc vgemm_big rebuild_big off Wdc+panel none")],
    "rebuild_tiles": [(1, 128, E_SMALL), (129, 175, E_SWEEP), (176, 255, E_PAD), (256, 256, E_256.replace("rebuild_big", "rebuild"))],
    "explicit_q": [(1, 128, E_SMALL), (129, 255, E_SWEEP),
                   (256, 256, "D half AR_FUSED panel+Q dc vgemm_big rebuild_big off Wdc+panel none")],
    "panel_one_stage": EIGEN_ONLY, "panel_two_stages": EIGEN_ONLY, "two_streams": EIGEN_ONLY, "dc_poison": EIGEN_ONLY,
    "spectral_two_streams": DEFAULT, "spectral_chunks": DEFAULT, "spectral_all_rejected": DEFAULT, "spectral_one_pass_cap": DEFAULT,
    "spectral_unfused": spectral("kernels", "kernels", "+spec_mat+spec_flag"),
    "spectral_no_fold": spectral("fused", "fused+late"),
    "streams_2": DEFAULT,
    # the matrix-function route follows the lean state: where ADMMNET_PAD_MIN keeps 128 < D < 256 off the 256 pipeline, both go
    "pad_min_150": DEFAULT[:2] + [(129, 149, E_SWEEP.replace("Wdc", "Wdc+spec_flag")), (150, 255, DEFAULT[2][2]), DEFAULT[3]],
    "pad_min_999": DEFAULT[:2] + [(129, 255, E_SWEEP.replace("Wdc", "Wdc+spec_flag")), DEFAULT[-1]],
}


def expected_row(name, D):
    (hit,) = [r for lo, hi, r in EXPECTED[name] if lo <= D <= hi]
    return hit


@pytest.mark.parametrize("name", list(ENVS))
def test_routes_at_the_edges(model, name):
    got = read_routes(model, ENVS[name], EDGES)
    assert [int(r["D"]) for r in got] == EDGES
    for r in got:
        assert row(r) == expected_row(name, int(r["D"])), (name, r["D"])


def test_anchor_routes(model):
    """The rows a reader of the parent can check by hand (ADMMNET_LEAN=0 keeps the padding from 129: the parent's pad_min
    looked at ADMMNET_SPECTRAL alone)."""
    def one(env, D):
        (r,) = read_routes(model, env, [D])
        return r
    for D in (100, 128):
        r = one({}, D)
        assert (r["storage"], r["first"], r["matfun"], r["fold"], r["tridiag"], r["rowmajor"], r["colmap"], r["rebuild"], r["back"]) == \
               ("lean", "AR_LDS", "fused", "1", "reg", "0", "0", "back_rebuild", "in_rebuild")
    assert {k: v for k, v in one({}, 7).items() if k not in ("D", "eig_dim", "matfun", "fold")} == \
           {k: v for k, v in one({}, 100).items() if k not in ("D", "eig_dim", "matfun", "fold")} and one({}, 7)["matfun"] == "off"
    for D in (130, 200, 255, 256):
        r = one({}, D)
        assert (r["eig_dim"], r["storage"], r["first"], r["matfun"], r["late_image"], r["tridiag"], r["explicit_q"], r["colmap"],
                r["back"], r["rebuild"]) == ("256", "half", "AR_FUSED", "fused", "1", "panel", "0", "1", "wy_apply", "rebuild_big")
    r = one({"ADMMNET_SPECTRAL": "0"}, 160)
    assert (r["eig_dim"], r["storage"], r["first"], r["matfun"], r["tridiag"], r["explicit_q"], r["back"], r["rebuild"]) == \
           ("160", "full", "AR_FUSED", "off", "sweep", "1", "vgemm_big", "rebuild")
    r = one({"ADMMNET_SPECTRAL": "0"}, 176)
    assert (r["eig_dim"], r["storage"], r["matfun"], r["tridiag"]) == ("256", "half", "off", "panel")
    r = one({"ADMMNET_LEAN": "0"}, 160)
    assert (r["eig_dim"], r["storage"], r["matfun"]) == ("256", "full", "off")


# ---- 3. self-consistency ------------------------------------------------------------------------------------------------------------
def test_every_route_is_consistent(model):
    """Every D in 1 .. 256 under every on/off combination of ADMMNET_EIG, SPECTRAL, SPECTRAL_FUSED, SF_FOLD, ARROW, ARROW_FUSED, LEAN,
    FUSE_BACK, TRIDIAG, TRIDIAG_BIG, BACK, REBUILD (bit i of the combination, in this order)."""
    v = np.frombuffer(model(["sweep"], {}, text=False), np.uint32).reshape(4096, 256).astype(np.int64)
    D = np.broadcast_to(np.arange(1, 257), v.shape)

    def f(shift, bits): return (v >> shift) & ((1 << bits) - 1)
    padded, storage, first, tridiag, q, dc, back, rebuild = f(0, 1), f(1, 2), f(3, 2), f(7, 2), f(9, 1), f(10, 1), f(11, 3), f(14, 2)
    matfun, late, fold, bufs, err, e256 = f(16, 2), f(18, 1), f(19, 1), f(20, 5), f(25, 2), f(27, 1)
    LEAN, HALF = 1, 2
    DENSE = 3
    REG, PANEL = 0, 3
    IN_REBUILD, VGEMM, VGEMM_BIG, WY, ROTATION = range(5)
    RB_BACK, RB_TILES = 0, 2
    FUSED, KERNELS = 1, 2
    WDC, LOG, PNL, SPEC_MAT, SPEC_FLAG = 1, 2, 4, 8, 16
    # the only refusal the parent's launchers could reach: the per-tile rebuild under the skip filter of the matrix-function route
    # (its lean loader and its five-kernel form were never handed a combination they refuse)
    assert set(np.unique(err)) <= {0, 1}
    assert np.array_equal(err == 1, (matfun != 0) & (rebuild == RB_TILES))
    assert np.all(D[err == 1] == 256)
    ok = err == 0
    # kernel -> chunk buffers it touches
    need = np.zeros_like(v)
    need |= np.where(dc == 1, WDC, LOG)                                   # dc_kernel: Wdc; tql + rotation replay: the log
    # (tridiag_panel_kernel takes Tfac and Tail when they exist -- null: no T factors stored, one stage; only wy_apply needs them)
    need |= np.where(back == WY, WDC | PNL, 0)                            # wy_apply: Wdc through Wmap, Tfac
    need |= np.where((back == VGEMM) | (back == VGEMM_BIG) | (back == IN_REBUILD), WDC, 0)
    need |= np.where(back == ROTATION, LOG, 0)
    need |= np.where(matfun == FUSED, SPEC_FLAG, 0)
    need |= np.where(matfun == KERNELS, SPEC_FLAG | SPEC_MAT, 0)
    need |= np.where(late == 1, SPEC_FLAG, 0)                             # half_image_kernel reads the flags
    assert np.all((need & ~bufs)[ok] == 0)
    assert np.all((rebuild == RB_BACK) == (back == IN_REBUILD))
    wy = ok & (back == WY)
    assert np.all((tridiag[wy] == PANEL) & (dc[wy] == 1) & (q[wy] == 0)) and np.all((q == 0) == (back == WY))
    big_lean = ok & (storage != 0) & (D > 128)
    assert np.all((storage[big_lean] == HALF) & (e256[big_lean] == 1) & (first[big_lean] != DENSE))
    assert np.all(storage[(D <= 128)] != HALF) and np.all(first[storage != 0] != DENSE)
    assert np.all((tridiag[storage == LEAN] == REG)) and np.all(tridiag[storage == HALF] == PANEL)
    mf = ok & (matfun != 0)
    assert np.all((storage[mf] != 0) & (D[mf] >= 8))
    assert np.all(matfun[fold == 1] == FUSED) and np.all(matfun[late == 1] == FUSED)
    assert np.all(e256[padded == 1] == 1) and np.all(D[padded == 1] > 128)


# ---- 4. workspace sizes --------------------------------------------------------------------------------------------------------------
GEOMS = [(2, 4), (10, 10), (8, 16), (3, 43), (10, 13), (10, 16), (7, 25), (11, 16), (12, 16), (15, 17), (16, 16)]
BATCHES = [(3, 0, 0), (5, 2, 2), (20000, 0, 0)]
SIZES_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
class Cfg(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("M", "N", "L", "K", "has_head", "chunk", "sub_batch", "reserved")]
for f in (lib.admmnet_workspace_bytes, lib.admmnet_glayer_workspace_bytes):
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.POINTER(Cfg), ctypes.c_int64]
lib.admmnet_eigh_workspace_bytes.restype, lib.admmnet_eigh_workspace_bytes.argtypes = ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64]
out = []
for M, N in json.loads(sys.argv[2]):
    for B, chunk, sub in json.loads(sys.argv[3]):
        cfg = Cfg(M, N, 3, 3, 0, chunk, sub, 0)
        out.append([lib.admmnet_workspace_bytes(ctypes.byref(cfg), B), lib.admmnet_glayer_workspace_bytes(ctypes.byref(cfg), B),
                    lib.admmnet_eigh_workspace_bytes(M * N + 1, B)])
print(json.dumps(out))
"""


def workspace_sizes(lib_path, env):
    p = subprocess.run([sys.executable, "-c", SIZES_CHILD, lib_path, json.dumps(GEOMS), json.dumps(BATCHES)], env=clean_env(env),
                       capture_output=True, text=True, check=True)
    return json.loads(p.stdout)


@pytest.mark.parametrize("name", list(ENVS))
def test_workspace_sizes_equal_the_parent(name):
    """admmnet_workspace_bytes / admmnet_glayer_workspace_bytes / admmnet_eigh_workspace_bytes per (geometry, batch) as the library
    built from the parent commit answered them (route_workspace_sizes.json; the calls need no GPU): carve_chunk byte for byte.
    An environment added later is recorded from the commit before it."""
    with open(SIZES) as fh:
        want = json.load(fh)[name]
    assert workspace_sizes(os.path.join(ROOT, "admm_net_amd", "libadmmnet_hip.so"), ENVS[name]) == want


# ---- 5. documentation ---------------------------------------------------------------------------------------------------------------
def test_switch_table_is_complete():
    with open(os.path.join(CSRC, "route.h")) as fh:
        src = fh.read()
    parsed = set(re.findall(r'"(ADMMNET_[A-Z_]+)"', src[src.index("inline Switches switches_from_env"):src.index("inline const Switches &switches")]))
    assert parsed == set(PARSE)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    sec = doc[doc.index("## 6."):]
    sec = sec[:sec.index("\n## ", 1)] if "\n## " in sec[1:] else sec
    assert set(re.findall(r"ADMMNET_[A-Z]+(?:_[A-Z]+)*", sec)) == parsed


def test_getenv_is_called_in_one_function():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f)) as fh:
            hits += [(f, i + 1) for i, ln in enumerate(fh) if re.search(r"\bgetenv\s*\(", ln)]
    assert len(hits) == 1 and hits[0][0] == "route.h", hits
