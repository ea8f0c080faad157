"""CPU suite (-m "not gpu"): the oracle against its pins, the C-ABI library's
exports, and the host logic of rampvo_amd (run over the oracle CPU backend)
against the golden vectors captured from the reference's own python."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle as orc
import pipeline_checks as pc
from oracle.backend_cpu import cpu_oracle_ops
from scenes import ba_scene, corr_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI surface
def test_library_loads_and_exports_every_declared_symbol():
    from rampvo_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    declared -= {"ramp_corr_level"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ramp_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert b"gfx950" in lib.ramp_version()


def _layout_mismatches(structs, tmp_path):
    """[(field, C's "offset size", ctypes')] where the system C compiler's sizeof / offsetof of a field the ctypes mirror
    names differs from the mirror's, field by field in the mirror's order; structs: (C name, ctypes.Structure) pairs"""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler on PATH"
    lines = ['#include "ramp_hip.h"', "#include <stdio.h>", "int main(void) {"]
    want = []
    for cname, py in structs:
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(py))
        for name, _ in py._fields_:
            lines.append('  printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, name, cname, name))
            want.append("%d %d" % (getattr(py, name).offset, getattr(py, name).size))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    names = [c for c, py in structs for c in [c] + ["%s.%s" % (c, n) for n, _ in py._fields_]]
    assert len(got) - 1 == len(want)
    return [(name, g, str(w)) for name, g, w in zip(names, got, want) if g != str(w)]


def test_track_descriptor_mirror_matches_the_c_layout(tmp_path):
    """track_dev.Track, _lib.TrackWeights / UpdateArgs / CorrLevel and conv_hip.ConvJob mirror include/ramp_hip.h's ramp_track /
    ramp_track_weights / ramp_update_args / ramp_corr_level / ramp_conv_job by hand: the system C compiler's sizeof and offsetof of every field
    the ctypes mirror names equal the ctypes ones, field by field in the mirror's order"""
    from rampvo_amd import _lib, conv_hip, track_dev
    assert track_dev.TrackWeights is _lib.TrackWeights
    assert "relu_t" not in [n for n, _ in track_dev.Track._fields_]
    structs = (("ramp_track", track_dev.Track), ("ramp_track_weights", _lib.TrackWeights),
               ("ramp_update_args", _lib.UpdateArgs), ("ramp_conv_job", conv_hip.ConvJob),
               ("ramp_corr_level", _lib.CorrLevel))
    for name, g, w in _layout_mismatches(structs, tmp_path):
        assert g == w, "%s: C %s, ctypes %s" % (name, g, w)


def test_update_args_layout_check_sees_a_swapped_field_pair(tmp_path):
    """the layout check above is not vacuous for ramp_update_args: a mirror with two neighbouring fields swapped (the
    last pointer, hij, and the first int, kk_cap) is reported for both"""
    from rampvo_amd import _lib
    fields = list(_lib.UpdateArgs._fields_)
    i, j = [n for n, _ in fields].index("hij"), [n for n, _ in fields].index("kk_cap")
    assert j == i + 1
    fields[i], fields[j] = fields[j], fields[i]
    swapped = type("SwappedUpdateArgs", (ctypes.Structure,), {"_fields_": fields})
    bad = _layout_mismatches((("ramp_update_args", swapped),), tmp_path)
    assert {"ramp_update_args.hij", "ramp_update_args.kk_cap"} <= {name for name, _, _ in bad}


def test_header_constants_equal_the_c_compilers_values(tmp_path):
    """every RAMP_* value macro _lib reads from include/ramp_hip.h has the value the system C compiler gives it (an f-suffixed
    literal: as a float32 on both sides), and the reader saw every `#define RAMP_` line that carries a value"""
    import shutil
    import subprocess
    from rampvo_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler on PATH"
    lines = [l.split() for l in open(_lib.HEADER) if l.startswith("#define RAMP_")]
    literal = {t[1]: t[2] for t in lines if len(t) > 2 and not t[2].startswith("/*")}
    assert sorted(literal) == sorted(_lib.CONSTANTS) and len(literal) > 100
    names = sorted(literal)
    src, exe = tmp_path / "constants.c", tmp_path / "constants"
    src.write_text('#include "ramp_hip.h"\n#include <stdio.h>\nint main(void) {\n' + "".join(
        '  printf("%%.17g\\n", (double)(%s));\n' % n for n in names) + "  return 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(got) == len(names)
    for n, g in zip(names, got):
        mine = _lib.CONSTANTS[n]
        assert getattr(_lib, n) is mine
        if isinstance(mine, int):
            assert float(g) == mine and float(g).is_integer(), (n, g, mine)
        elif literal[n][-1] in "fF":
            assert np.float32(float(g)) == np.float32(mine), (n, g, mine)
        else:
            assert float(g) == mine, (n, g, mine)
    assert _lib.RAMP_WARP_MIN_Z == 0.2 and _lib.RAMP_RECTIFY_TOL == 2.0 ** -6 and _lib.RAMP_CORR_X2 == 128
    assert {rc: text.split()[0] for rc, text in _lib._ERR.items()} == {
        _lib.RAMP_EINVAL: "RAMP_EINVAL", _lib.RAMP_ELAUNCH: "RAMP_ELAUNCH", _lib.RAMP_EWORKSPACE: "RAMP_EWORKSPACE",
        _lib.RAMP_EUNSUPPORTED: "RAMP_EUNSUPPORTED"}


_SYNTHETIC_HEADER = """
#define RAMP_SYN_H
#define RAMP_SYN_A 3
#define RAMP_SYN_B -0x10  /* a comment that runs
                             over two lines */
#define RAMP_SYN_C 0.25f
/* int ramp_syn_commented(int a); */
typedef struct ramp_syn_thing {
  int a;          /* ramp_syn_field(int x); */
  const void *p;
} ramp_syn_thing;
const char *ramp_syn_name(void);
size_t ramp_syn_bytes(const float *x, void *y, const ramp_syn_thing *const *t, int a, int32_t b, int64_t c);
long ramp_syn_many(long a, size_t b,
                   uint32_t c, float d, /* optional */
                   double e, const int v[3]);
"""


def test_header_reader_on_a_synthetic_header():
    """_lib.parse_header on a header with one parameter of every kind: exactly the expected constants and signatures, nothing
    from a comment or a struct body, and a type or a literal it does not know raises (nothing defaults to int)"""
    from rampvo_amd import _lib
    c = ctypes
    constants, signatures = _lib.parse_header(_SYNTHETIC_HEADER)
    assert constants == {"RAMP_SYN_A": 3, "RAMP_SYN_B": -16, "RAMP_SYN_C": 0.25}
    assert [type(constants[k]) for k in ("RAMP_SYN_A", "RAMP_SYN_B", "RAMP_SYN_C")] == [int, int, float]
    assert signatures == {
        "ramp_syn_name": (c.c_char_p, []),
        "ramp_syn_bytes": (c.c_size_t, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int32, c.c_int64]),
        "ramp_syn_many": (c.c_long, [c.c_long, c.c_size_t, c.c_uint32, c.c_float, c.c_double, c.c_void_p])}
    for bad in ("int ramp_syn_bad(short a);", "int ramp_syn_bad(int);", "short ramp_syn_bad(int a);",
                "void *ramp_syn_bad(int a);", "#define RAMP_SYN_BAD (1 << 3)\n", "#define RAMP_SYN_BAD(x) 3\n"):
        with pytest.raises(RuntimeError):
            _lib.parse_header(bad)


def test_header_reader_on_the_whole_header():
    """every ramp_* declaration the export test finds has a signature and there is no other; four of the longest argument
    lists, written out here by hand from the header text (p pointer, i int, l long, z size_t, f float, d double)"""
    from rampvo_amd import _lib
    header = open(_lib.HEADER).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header)) - {"ramp_corr_level"}
    assert len(declared) > 100 and declared <= set(_lib.SIGNATURES)
    assert set(re.findall(r"\b(ramp_\w+)\s*\(", header)) == set(_lib.SIGNATURES)       # (\w: ramp_se3_adjT has a capital)
    letter = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "z": ctypes.c_size_t, "f": ctypes.c_float,
              "d": ctypes.c_double}
    for name, args in (("ramp_event_warp", "pppp i pp i d pp iiii ppppp z pp"),
                       ("ramp_invdepth_map", "pppp iii f pp i p ii pp ff iii pppp z pp"),
                       ("ramp_event_filter", "ppp l iii dd i d ppppppppppp z p"),
                       ("ramp_imu_propagate", "ppp l ppp dd i ppppp z p")):
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and argtypes == [letter[a] for a in args.replace(" ", "")], name
    assert len(_lib.SIGNATURES["ramp_event_warp"][1]) == 23 and _lib.SIGNATURES["ramp_event_warp"][1][8] is ctypes.c_double
    assert len(_lib.SIGNATURES["ramp_invdepth_map"][1]) == 28
    assert _lib.SIGNATURES["ramp_version"] == (ctypes.c_char_p, [])
    assert _lib.SIGNATURES["ramp_event_warp_grid_events"] == (ctypes.c_long, [])
    assert _lib.SIGNATURES["ramp_stream_signal"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]


def test_a_missing_header_is_named(monkeypatch, tmp_path):
    from rampvo_amd import _lib
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "nowhere" / "ramp_hip.h"))
    with pytest.raises(RuntimeError, match="nowhere"):
        _lib._read_header()


def test_gru_tile_rows_follow_the_round_rule_at_its_edges():
    """ramp_upd_gru_tile_rows is the rule ramp_upd_gru's launch applies (one function in csrc/update_mlp.hip) and the one
    the frame pipeline asks when it places the next front end around that launch.  Restated here in integers: 64- or 80-row
    tiles, whichever needs fewer rounds of one workgroup per CU counted in 16-row units (4 or 5 per round), a tie gives 64;
    a positive E_hint below E stands in for E.  CU count: the device's, 256 without one (the launcher's fallback)."""
    from rampvo_amd import _lib
    rows = _lib.lib().ramp_upd_gru_tile_rows
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256
    cdiv = lambda a, b: (a + b - 1) // b

    def want(E, hint=0):
        live = hint if 0 < hint < E else E
        return 80 if cdiv(cdiv(live, 80), cus) * 5 < cdiv(cdiv(live, 64), cus) * 4 else 64

    edges = sorted({1, 63, 64, 65, 80, 81} | {t * cus * k + d for t in (64, 80) for k in (1, 2, 3, 4, 5) for d in (-1, 0, 1)})
    for E in edges:
        assert rows(E, 0) == want(E), (E, cus)
        for hint in (0, -5, 1, E - 1, E, E + 1, 64 * cus, 64 * cus + 1, 80 * cus, 80 * cus + 1):
            assert rows(E, hint) == want(E, hint), (E, hint, cus)
    assert want(320 * cus) == 64 and rows(320 * cus, 0) == 64           # five rounds of 64 rows = four of 80: the tie
    assert rows(80 * cus + 1, 80 * cus) == 80 and rows(80 * cus + 1, 0) == 64 and rows(80 * cus, 80 * cus + 1) == 80
    if cus == 256:
        table = {1: 64, 16384: 64, 16385: 80, 20480: 80, 20481: 64, 32768: 64, 32769: 80, 40960: 80, 40961: 64}
        assert {E: rows(E, 0) for E in table} == table
        assert rows(81920, 0) == 64                                     # 20 = 20
        assert rows(46000, 40960) == 80 and rows(46000, 0) == 64 and rows(46000, 46000) == 64 and rows(40960, 46000) == 80


def test_switch_reader_defaults_and_fallbacks():
    """rampvo_amd.switches.read(): unset variables give the defaults, values that do not parse or are out of range give
    the same defaults, and kernel-serialising runtimes turn the flag waits off"""
    from rampvo_amd import _lib, switches
    d = switches.read({})
    assert d == switches.Switches()
    assert (d.device_step, d.inputs_ready, d.flag_waits, d.x3, d.conv_x3, d.corr_f32_mfma, d.host_threads) == \
        (True, False, True, True, True, 2, None)
    junk = switches.read(dict(RAMP_DEVICE_STEP="yes", RAMP_INPUTS_READY="maybe", RAMP_NO_FLAG_WAITS="0", RAMP_X3="on",
                              RAMP_CONV_X3="", RAMP_CORR_F32_MFMA="fast", RAMP_HOST_THREADS="many"))
    assert junk == switches.Switches(device_step=False, x3=False)      # (only "1" turns these two on)
    assert switches.read(dict(RAMP_CORR_F32_MFMA="7")).corr_f32_mfma == 2
    assert switches.read(dict(RAMP_CORR_F32_MFMA="-1")).corr_f32_mfma == 2
    assert switches.read(dict(RAMP_HOST_THREADS="-3")).host_threads is None
    assert switches.read(dict(RAMP_HOST_THREADS="")).host_threads is None
    s = switches.read(dict(RAMP_DEVICE_STEP="0", RAMP_INPUTS_READY="stream", RAMP_X3="0", RAMP_CONV_X3="0",
                           RAMP_CORR_F32_MFMA="0", RAMP_HOST_THREADS="0"))
    assert s == switches.Switches(device_step=False, inputs_ready="stream", x3=False, conv_x3=False, corr_f32_mfma=0,
                                  host_threads=0)
    assert switches.read(dict(RAMP_INPUTS_READY="1", RAMP_CORR_F32_MFMA="1", RAMP_HOST_THREADS="6")) == \
        switches.Switches(inputs_ready=True, corr_f32_mfma=1, host_threads=6)
    for k in ("RAMP_NO_FLAG_WAITS", "ROCPROF_COUNTER_COLLECTION", "AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING"):
        assert not switches.read({k: "1"}).flag_waits and switches.read({k: "0"}).flag_waits
    assert _lib.corr_f32_mode() == switches.read().corr_f32_mfma


def test_switches_are_read_in_one_place():
    """the C library reads no environment (every choice is an argument or a ramp_track field), and in the package only
    the switch reader, _lib.LIB_PATH (RAMP_HIP_LIB) and hostenv's LOCAL_WORLD_SIZE touch os.environ"""
    csrc = os.path.join(ROOT, "rampvo_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    allowed = {"switches.py": None, "_lib.py": "RAMP_HIP_LIB", "hostenv.py": "LOCAL_WORLD_SIZE"}
    pkg = os.path.join(ROOT, "rampvo_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py") or os.path.join(dirpath, f) == os.path.join(pkg, "switches.py"):
                continue
            for line in open(os.path.join(dirpath, f)):
                if "environ" in line or "getenv" in line:
                    assert dirpath == pkg and allowed.get(f) and allowed[f] in line, (f, line)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rampvo_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), f
                assert "ramp_oracle" not in src and "liboracle" not in src, f


def test_ops_have_no_cpu_fallback():
    from rampvo_amd import ops
    with pytest.raises(RuntimeError):
        ops.se3_unary("ramp_se3_inv", torch.zeros(1, 7), 7, 7)
    with pytest.raises(RuntimeError):
        ops.group_by(torch.zeros(4, dtype=torch.int64))


def test_product_modules_and_tracker_refuse_cpu():
    """no ATen / CPU path inside the package: the encoder, the update operator and the tracker run their HIP
    kernels or raise (the torch restatements used by these CPU tests live in oracle/host_cpu.py)"""
    from rampvo_amd.config import make_cfg
    from rampvo_amd.Ramp_vo import Ramp_vo
    from rampvo_amd.synthetic import make_network
    assert not os.path.exists(os.path.join(ROOT, "rampvo_amd", "conv.py"))
    net = make_network("SingleScale", device="cpu")
    with pytest.raises(RuntimeError):
        net.patchify.encoder(events=torch.zeros(1, 1, 5, 32, 32), images=torch.zeros(1, 1, 3, 32, 32))
    with pytest.raises(RuntimeError):
        net.update(torch.zeros(1, 4, 384), torch.zeros(1, 4, 384), torch.zeros(1, 4, 882), None,
                   torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        make_network("MultiScale", device="cpu").patchify.encoder(
            events=torch.zeros(1, 1, 5, 32, 32), images=torch.zeros(1, 1, 3, 32, 32), mask=torch.tensor([True]))
    with pytest.raises(RuntimeError):
        Ramp_vo(make_cfg("default"), net, {"event_bias": True}, device="cpu")


# ----------------------------------------------------------------- oracle pins
def test_oracle_se3_identities_of_reference_run_tests():
    """ramp/lietorch/run_tests.py:16-52 (exp/log, inverse, adjoint, act == matrix) at fp32"""
    rng = np.random.default_rng(0)
    a = (0.2 * rng.normal(size=(200, 6))).astype(np.float32)
    X = orc.se3_exp(a)
    assert np.abs(orc.se3_log(X) - a).max() < 2e-6
    assert np.abs(orc.se3_log(orc.se3_mul(X, orc.se3_inv(X)))).max() < 2e-6
    c = rng.normal(size=(200, 6)).astype(np.float32)
    Xb = orc.se3_exp(rng.normal(size=(200, 6)).astype(np.float32))
    Y1 = orc.se3_mul(Xb, orc.se3_exp(c))
    Y2 = orc.se3_mul(orc.se3_exp(orc.se3_adj(Xb, c)), Xb)
    assert np.abs(orc.se3_log(orc.se3_mul(Y1, orc.se3_inv(Y2)))).max() < 3e-5
    # act4 == 4x4 matrix (columns = action on the basis) applied to the point
    p = rng.normal(size=(200, 4)).astype(np.float32)
    I = np.eye(4, dtype=np.float32)
    Mx = np.stack([orc.se3_act4(Xb, np.broadcast_to(I[k], (200, 4))) for k in range(4)], -1)
    assert np.abs(orc.se3_act4(Xb, p) - np.einsum("nij,nj->ni", Mx, p)).max() < 1e-5
    # adjT is the transpose of adj
    b = rng.normal(size=(200, 6)).astype(np.float32)
    lhs = (orc.se3_adj(Xb, c) * b).sum(-1)
    rhs = (c * orc.se3_adjT(Xb, b)).sum(-1)
    assert np.abs(lhs - rhs).max() < 2e-4 * np.abs(lhs).max()


def test_oracle_corr_against_dense_einsum():
    fmap1, fmap2, coords, ii, jj = corr_case(seed=1, E=12, distort=False)
    coords[0, 3] = coords[0, 2]
    coords[0, 5] = coords[0, 4]
    out = orc.corr(fmap1, fmap2, coords, ii, jj, 3)[0]
    H, W = fmap2.shape[-2:]
    for e in range(12):
        full = np.einsum("cp,chw->phw", fmap1[0, ii[e]].reshape(128, 9).astype(np.float64),
                         fmap2[0, jj[e]].astype(np.float64))
        pad = np.zeros((9, H + 40, W + 40))
        pad[:, 20:20 + H, 20:20 + W] = full
        for p in range(9):
            x, y = coords[0, e, 0].reshape(9)[p], coords[0, e, 1].reshape(9)[p]
            fx, fy = int(np.floor(x)), int(np.floor(y))
            dx, dy = x - fx, y - fy
            win = pad[p, 20 + fy - 3:20 + fy + 5, 20 + fx - 3:20 + fx + 5]        # [8(y), 8(x)]
            ref = ((1 - dx) * (1 - dy) * win[:7, :7] + dx * (1 - dy) * win[:7, 1:] + (1 - dx) * dy * win[1:, :7]
                   + dx * dy * win[1:, 1:])
            got = out[e, :, :, p // 3, p % 3]                                         # [x-off, y-off]
            assert np.abs(got - ref.T).max() < 2e-4


def test_oracle_ba_fp64_pin_against_reference_python_ba_and_jacobians():
    """The tight, independent pin of the bundle-adjustment restatement (oracle/ramp_oracle.c::ba_impl / ba_edge_terms, after
    ramp/fastba/ba_cuda.cu:232-376, 433-582).  Fixture ba_f64_pin.npz = the reference's OWN python in FLOAT64 -- ramp/ba.py::BA
    (ep = 1.0) and ramp/projective_ops.py::transform(jacobian=True), oracle/make_golden.py::gen_ba_f64_pin -- on branch-free
    problems (tests/scenes.py::ba_pin_scene), 10 and 30 free poses, one and two Gauss-Newton steps.  The fp64 build of the
    oracle source must reproduce: Jacobians (Ji with the kernel's folded sign, Jj, Jz) to 1e-10 relative, poses / depths
    after the solve to 1e-8.  One stated exception, the reference kernel's own: expSE3 (ba_cuda.cu:140) adds the rotational
    part of the translation update only `if (theta > 1e-4)`, python's retraction is the exact exponential -- a pose whose
    rotation step is below 1e-4 may differ by 0.5e-4 |translation step| (seen on the second step of the 10-pose window:
    1.2e-8 on a 3e-4 step); quaternions and depths are not affected and stay within 1e-8."""
    from scenes import ba_pin_scene
    from oracle.make_golden_params import BA_PIN
    g = pc.gold("ba_f64_pin.npz")
    for tag, kw in BA_PIN.items():
        s = ba_pin_scene(**kw)
        n = s["n_frames"]
        et = orc.ba_edge_terms(s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"], f64=True)
        for name, got in (("Ji", -et["Ji"]), ("Jj", et["Jj"]), ("Jz", et["Jz"])):
            ref = g["%s_%s" % (tag, name)]
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (tag, name)
        prev = s["poses"]
        for steps in (1, 2):
            p64, pt64 = orc.ba_f64(s["poses"], s["patches"], s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"],
                                   s["kk"], 1, n, steps)
            rp, rd = g["%s_poses_%d" % (tag, steps)], g["%s_depths_%d" % (tag, steps)]
            step_t = np.abs(rp[:, :3] - prev[:, :3]).max()
            assert np.abs(rp - s["poses"]).max() > 1e-3                                   # (a real step was taken)
            assert np.abs(p64[:, 3:] - rp[:, 3:]).max() <= 1e-8, (tag, steps)
            assert np.abs(pt64[:, 2, 1, 1] - rd).max() <= 1e-8, (tag, steps)
            assert np.abs(p64[:, :3] - rp[:, :3]).max() <= 1e-8 + 0.5e-4 * step_t, (tag, steps)
            if steps == 1:
                assert np.abs(p64[:, :3] - rp[:, :3]).max() <= 1e-8, tag                # (first steps rotate by > 1e-4)
            prev = rp
        # and the fp32 restatement (the parity oracle itself) is the same SOURCE: within the fp32 rounding envelope of these
        # gauge-weak problems (measured 3e-3 of the step on the 10-pose window, 1e-3 on the 30-pose one) of its fp64 twin
        p32, pt32 = s["poses"].astype(np.float32), s["patches"].astype(np.float32)
        orc.ba(p32, pt32, s["intr"].astype(np.float32), s["target"].astype(np.float32), s["weight"].astype(np.float32),
               s["lmbda"].astype(np.float32), s["ii"], s["jj"], s["kk"], 1, n, 2)
        step = np.abs(g["%s_poses_2" % tag] - s["poses"]).max()
        assert np.abs(p32 - g["%s_poses_2" % tag]).max() <= 6e-3 * step, tag
        assert np.abs(pt32[:, 2, 1, 1] - g["%s_depths_2" % tag]).max() <= 5e-4, tag          # (the scale gauge: all depths move together)


def test_oracle_ba_crosscheck_with_reference_python_ba():
    """fixture ba_crosscheck.npz: the reference's own python ramp/ba.py::BA (run in the build container)
    against the C restatement of cuda_ba on the same problem, one GN step"""
    g = pc.gold("ba_crosscheck.npz")
    step = float(g["moved"])
    assert np.abs(g["poses_python"] - g["poses_oracle"]).max() < 2e-3 * step + 1e-6
    assert np.abs(g["patches_python"][:, 2] - g["patches_oracle"][:, 2]).max() < 1e-4
    # and the oracle reproduces its own recorded result (the fixture is not stale)
    s = ba_scene(seed=21, n_frames=8, M=10, lifetime=4, noise=0.8, n_total_frames=8)
    c = orc.transform(s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])[0][:, :, 1, 1]
    bad = np.linalg.norm(s["target"] - c, axis=1) > 50
    s["target"][bad] = c[bad]
    p, pt = s["poses"].copy(), s["patches"].copy()
    orc.ba(p, pt, s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], 1, 8, 1)
    assert np.array_equal(p, g["poses_oracle"]) and np.array_equal(pt, g["patches_oracle"])


def test_oracle_event_stack_against_reference_golden():
    """oracle.event_stack == the reference's EventToStack_Numpy output frozen by oracle/make_golden.py"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "event_stack.npz"))
    out = orc.event_stack(g["x"], g["y"], g["p"], int(g["height"]), int(g["width"]), int(g["bins"]))
    assert out.dtype == np.int8 and np.array_equal(out, g["out"])
    assert out[0, 9, 7] == 45          # 301 events on one pixel wrap to 45, as upstream


def test_host_graph_edit_matches_numpy_logic():
    """libramp_hip.so's HOST helper ramp_graph_edit_host (one C pass) against the oracle-side tracker's _graph_edit (the
    numpy restatement of reference Ramp_vo.py:247-274 + :203-208), both outcomes of the motion test"""
    import ctypes
    from oracle.host_cpu import RampVoCPU
    from rampvo_amd import _lib
    rng = np.random.default_rng(3)
    M, n, R, KI = 8, 30, 22, 4
    fake = type("T", (), {})()
    fake.cfg = type("C", (), dict(KEYFRAME_INDEX=KI, REMOVAL_WINDOW=R))()
    fake.M, fake.n = M, n
    kk = np.sort(rng.integers(0, n * M, 5000)).astype(np.int64)
    fake._kk, fake._ii = kk, kk // M
    fake._jj = rng.integers(0, n, 5000).astype(np.int64)
    rows = rng.permutation(5000).astype(np.int64)
    for remove in (True, False):
        ref = RampVoCPU._graph_edit(fake, remove)
        out = np.empty((4, 5000), np.int64)
        rng_out = np.empty(4, np.int64)
        k = n - KI if remove else -1
        m = _lib.lib().ramp_graph_edit_host(fake._ii.ctypes.data, fake._jj.ctypes.data, fake._kk.ctypes.data,
                                            rows.ctypes.data, 5000, M, k, ref["n"], R, out.ctypes.data, 5000,
                                            rng_out.ctypes.data)
        assert m == len(ref["ii"]) and ref["changed"]
        assert rng_out.tolist() == [ref["kk"].min(), ref["kk"].max(), min(ref["ii"].min(), ref["jj"].min()),
                                    max(ref["ii"].max(), ref["jj"].max())]
        assert np.array_equal(out[0, :m], ref["ii"]) and np.array_equal(out[1, :m], ref["jj"])
        assert np.array_equal(out[2, :m], ref["kk"]) and np.array_equal(out[3, :m], rows[ref["idx"]])


@pytest.mark.parametrize("window", ["window", "all_free"])
def test_oracle_eff_impl_lookup_equals_dense(window):
    """the oracle's restatement of the reference's ``eff_impl=True`` path (block-sparse E behind a per-frame block
    table, fastba/block_e.cu:43-283: ``orc.ba(eff_ppf=M)``) against its restatement of the dense path
    (fastba/ba_cuda.cu:433-582): the same Gauss-Newton step, so the two agree to fp32 rounding -- which is what lets
    the product serve ``eff_impl`` from one storage"""
    M = 14
    s = ba_scene(seed=5, n_frames=9, M=M, lifetime=4, n_total_frames=12)
    nf = s["n_frames"]
    t0, t1 = (nf - 5, nf) if window == "window" else (1, nf)
    out = []
    for ppf in (0, M):
        p, pt = s["poses"].copy(), s["patches"].copy()
        st = orc.ba(p, pt, s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], t0, t1, 2, eff_ppf=ppf)
        assert st == 0
        out.append((p, pt))
    step = np.abs(out[0][0] - s["poses"]).max()
    assert step > 1e-4
    tol = 1e-5 if window == "window" else 2e-4        # all_free: gauge freedom, the ill-conditioned case of the GPU test
    assert np.abs(out[0][0] - out[1][0]).max() <= tol * max(1.0, step)
    assert np.abs(out[0][1] - out[1][1]).max() <= 10 * tol * max(1.0, np.abs(out[0][1][:, 2]).max())


def test_oracle_ba_properties():
    s = ba_scene(seed=5, n_frames=8, M=10, lifetime=4)
    p, pt = s["poses"].copy(), s["patches"].copy()
    assert orc.ba(p, pt, s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], 3, 8, 2) == 0
    assert np.array_equal(p[:3], s["poses"][:3])                     # fixed poses untouched
    assert np.array_equal(pt[:, :2], s["patches"][:, :2])            # only the depth channel moves
    assert np.all(pt[:, 2] >= 1e-4) and np.all(pt[:, 2] <= 20.0)     # clamps of patch_retr_kernel
    assert np.abs(np.linalg.norm(p[:, 3:], axis=1) - 1).max() < 1e-5
    # zero weights: structure and poses stay put up to the damping (dX = 0, dZ = 0)
    p2, pt2 = s["poses"].copy(), s["patches"].copy()
    orc.ba(p2, pt2, s["intr"], s["target"], 0 * s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], 3, 8, 2)
    assert np.abs(p2 - s["poses"]).max() < 1e-6 and np.abs(pt2 - s["patches"]).max() < 1e-6
    # empty graph is a no-op
    e = np.zeros(0, np.int64)
    p3 = s["poses"].copy()
    orc.ba(p3, s["patches"].copy(), s["intr"], np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32),
           s["lmbda"], e, e, e, 3, 8, 2)
    assert np.array_equal(p3, s["poses"])


def test_oracle_neighbors_and_softagg_small():
    kk = np.array([3, 3, 1, 3, 1, 7], np.int64)
    jj = np.array([5, 2, 0, 2, 0, 1], np.int64)
    ix, jx = orc.neighbors(kk, jj)
    assert ix.tolist() == [3, -1, -1, 1, 2, -1] and jx.tolist() == [-1, 3, 4, 0, -1, -1]
    rng = np.random.default_rng(0)
    fx, gx = rng.normal(size=(6, 4)).astype(np.float32), rng.normal(size=(6, 4)).astype(np.float32)
    uk, inv = np.unique(kk, return_inverse=True)
    y = orc.segment_softmax_sum(fx, gx, inv, len(uk))
    for g in range(len(uk)):
        w = np.exp(gx[inv == g] - gx[inv == g].max(0))
        w /= w.sum(0)
        assert np.abs(y[g] - (fx[inv == g] * w).sum(0)).max() < 1e-6


# ------------------------------------------- host logic vs reference goldens (CPU)
@pytest.mark.parametrize("mode", ["SingleScale", "MultiScale"])
def test_patchify_against_reference_golden_cpu(mode):
    with cpu_oracle_ops():
        worst = pc.check_patchify(mode, "cpu", tol=2e-4)
    print(worst)


def test_update_operator_against_reference_golden_cpu():
    with cpu_oracle_ops():
        print(pc.check_update("cpu", tol=2e-4))


def test_ramp_vo_against_reference_golden_cpu():
    """the whole state machine (init, motion probe, 12 init updates, update+keyframe per frame, terminate)"""
    with cpu_oracle_ops():
        print(pc.check_ramp_vo("cpu"))


def test_update_step_teacher_forced_cpu():
    """one update() from the reference's captured state vs the reference's own update()"""
    with cpu_oracle_ops():
        e = pc.check_update_step("cpu")
    print(e)
    scale = max(1.0, e["step"])
    assert e["weight"] <= 1e-5 and e["net"] <= 1e-5
    assert e["poses"] <= 1e-4 * scale and e["depths"] <= 1e-4 * scale and e["points"] <= 2e-2
    for k, v in e.items():
        if k.startswith("kf"):
            assert v <= 1e-5, (k, v)


def test_vo_state_roundtrip_cpu():
    """state_dict() / load_state_dict(): a restored tracker continues identically"""
    with cpu_oracle_ops():
        from oracle.backend_cpu import Ramp_vo as cpu_tracker
        from rampvo_amd.config import make_cfg
        from rampvo_amd.synthetic import SyntheticStream, make_network
        cfg = make_cfg("default", PATCHES_PER_FRAME=8, MIXED_PRECISION=False)
        net = make_network("SingleScale", device="cpu")
        a = cpu_tracker(cfg, net, {"event_bias": True}, ht=64, wd=96)
        stream = SyntheticStream(64, 96, 12, seed=3)
        torch.manual_seed(0)
        for t in range(10):
            im, ev, K, mask = stream.frame(t)
            a(t, input_tensor=(ev, im, mask), intrinsics=K)
        b = cpu_tracker(cfg, net, {"event_bias": True}, ht=64, wd=96)
        b.load_state_dict(a.state_dict())
        a.update()
        b.update()
        assert torch.equal(a.poses_, b.poses_) and torch.equal(a.patches_, b.patches_) and torch.equal(a.net, b.net)


def test_pose_prediction_helpers_against_reference_golden():
    """rampvo_amd.pose_prediction helpers vs the reference's own helpers (tests/golden/pose_pred.npz, generated
    by oracle/make_golden.py::gen_pose_pred from ramp/pose_prediction/pose_pred_utils.py on the reference
    tracker's state): appended factors, patch tracks, and the coords / weights written by the spline models."""
    import torch
    from rampvo_amd.pose_prediction import pose_pred_utils as pp
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_pred.npz"))
    n, M, r = int(g["n"]), int(g["M"]), int(g["r"])
    T = lambda k: torch.from_numpy(g[k])          # noqa: E731
    with cpu_oracle_ops():       # SE3 ops on CPU tensors exist only through the oracle backend
        boot = pp.motion_bootstrap(n=n, poses=T("poses_in")[0], MOTION_MODEL="DAMPED_LINEAR", MOTION_DAMPING=0.5)
    assert np.abs(boot.numpy() - g["boot"]).max() <= 1e-6
    ii, jj, kk, w = pp.add_forward_elements(frame_num=n + 1, patch_extracted_num=M, r=r, ii=T("ii"), jj=T("jj"),
                                            kk=T("kk"), ix=T("ix"), weights=T("last_weight").clone())
    assert np.array_equal(ii.numpy(), g["ii2"]) and np.array_equal(jj.numpy(), g["jj2"])
    assert np.array_equal(kk.numpy(), g["kk2"]) and tuple(w.shape) == tuple(g["w_up_shape"])
    coords = T("coords_in").clone()
    tracks = pp.compute_patch_track__(coords=coords, ii=ii, jj=jj, kk=kk, image_to_proj=n)
    assert np.array_equal(np.array(list(tracks.keys()), np.int64), g["track_keys"])
    assert np.array_equal(np.array([len(v) for v in tracks.values()]), g["track_lens"])
    assert np.array_equal(np.concatenate([v.numpy() for v in tracks.values()], 0), g["track_xy"])
    models = pp.fit_model_patch_track(next_frame_index=n, patch_dict=tracks, img_to_keyframe_map=T("tstamps"), ii=ii,
                                      jj=jj, data_shape=(int(g["ht"]), int(g["wd"])), frequency=int(g["frequency"]),
                                      deg=int(g["deg"]))
    c2, w2 = pp.predict_patch_on_model(patch_models=models, step_to_pred_future=int(g["step"]),
                                       frequency=int(g["frequency"]), next_frame_index=n, coords=coords, weights=w,
                                       ii=ii, jj=jj, kk=kk)
    assert c2 is coords and w2 is w                                   # in place, as upstream
    assert np.array_equal(w.numpy(), g["weights_out"])
    assert np.array_equal(coords.numpy(), g["coords_out"])            # same FITPACK, same arithmetic: bit equal
    # channel 0 = x everywhere else in the code base; the opt-out writes that instead
    c3, _ = pp.predict_patch_on_model(models, int(g["step"]), int(g["frequency"]), n, T("coords_in").clone(), w, ii, jj,
                                      kk, reference_layout=False)
    ch = (g["coords_out"] != g["coords_in"]).any(axis=(0, 2, 3, 4))
    assert np.array_equal(c3.numpy()[0, ch, 0, :, 0], g["coords_out"][0, ch, 1, :, 0])      # x along rows
    assert np.array_equal(c3.numpy()[0, ch, 1, 0, :], g["coords_out"][0, ch, 0, 0, :])      # y along columns


def test_ate_metric_and_writers(tmp_path):
    """ATE = RMS position error after Sim(3) alignment (what evo's ape(align=True, correct_scale=True) reports,
    reference evaluate.py:295-304): zero for any similarity transform of the same path, the plain RMS of the noise
    otherwise; the TUM-style and COLMAP writers produce the reference's file layouts."""
    from rampvo_amd import evaluate as ev
    rng = np.random.default_rng(5)
    ref = np.cumsum(rng.normal(size=(50, 3)), 0)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A *= np.sign(np.linalg.det(A))
    est = (ref - 3.0) @ A.T / 2.5 + np.array([1.0, -2.0, 0.5])
    assert ev.ate_rmse(est, ref) < 1e-9
    s, R, t = ev.umeyama_sim3(est, ref)
    assert abs(s - 2.5) < 1e-9 and np.allclose(R, A.T, atol=1e-9)
    noisy = ref + rng.normal(scale=0.01, size=ref.shape)
    assert 0.005 < ev.ate_rmse(noisy, ref) < 0.03
    poses = np.concatenate([ref, np.tile([0.0, 0.0, 0.0, 1.0], (50, 1))], 1)          # tx ty tz qx qy qz qw
    tr = ev.Trajectory.from_terminate(poses, np.arange(50) * 1e9)
    assert tr.num_poses == 50 and np.array_equal(tr.orientations_quat_wxyz[0], [1, 0, 0, 0])
    d = ev.save_results(tr, tr, "scene", root=str(tmp_path))
    got = np.loadtxt(os.path.join(d, "stamped_traj_estimate.txt"))
    assert got.shape == (50, 8) and np.allclose(got[:, 0], np.arange(50)) and np.allclose(got[:, 1:4], ref)
    c = ev.save_output_for_COLMAP(str(tmp_path / "colmap"), tr, ref[:5], np.full((5, 3), 0.5), 320, 320, 320, 240)
    assert (c / "cameras.txt").read_text() == "1 PINHOLE 640 480 320 320 320 240"
    assert len((c / "points3D.txt").read_text().splitlines()) == 5
    assert (c / "images.txt").read_text().splitlines()[0].startswith("1 1.0 0.0 0.0 0.0 ")


@pytest.mark.parametrize("tag", ["ss", "ms"])
def test_trajectory_against_reference_run_cpu(tag):
    """free-running tracker (damped weights) over the oracle backend vs the reference's own run: the host logic
    (edges, keyframe shuffle, ring-buffer aliasing at n > 32 in "ms") reproduces the reference's trajectory"""
    with cpu_oracle_ops():
        e = pc.check_trajectory(tag, "cpu")
    print(e)
    assert e["rel"] <= 1e-5 and e["depths_rel"] <= 1e-4, e
    if tag == "ms":
        assert e["jj_max"] >= 45      # the frame index wrapped the 32-slot ring


def test_oracle_corr_against_reference_call_site_golden():
    """G3: orc.corr on both pyramid levels, stacked as Ramp_vo.corr stacks them, equals what the reference's
    altcorr.corr python call site returned in the build container"""
    from scenes import corr_case
    g = pc.gold("corr.npz")
    f1, f2, coords, ii, jj = corr_case(seed=int(g["seed"]), E=int(g["E"]))
    c1 = orc.corr(f1, f2, coords / 1, ii, jj, 3)
    c2 = orc.corr(f1, g["fmap2_l1"].astype(np.float32), coords / 4, ii, jj, 3)
    out = np.stack([c1, c2], -1).reshape(1, len(ii), -1)
    assert out.shape == g["out"].shape and np.array_equal(out, g["out"])


def test_split_fp16_planes_host_restatement():
    """fp32 features as two fp16 parts (RAMP_CORR_X2; csrc/altcorr.hip::corr_split2): the torch restatement the GPU test checks
    the pack kernel against (ops.pack_split) -- layout [H][4][2][W][32] inside the float32 container, hi = fp16(x) (0 below the
    fp16 normal range), lo = fp16((x - hi) 2^11), hi + lo 2^-11 within 2^-22 |x| (11 bits of x for the tiny values), and a
    re-split of the decoded value is the same value (load_state_dict(state_dict()) keeps the planes' values)"""
    import torch
    from rampvo_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 16, 128, generator=g) * 0.7
    x[0, 0, 0, :6] = torch.tensor([1e-6, -3e-5, 6.2e-5, 0.0, 65000.0, -1e-9])
    c = ops.pack_split(x)
    assert c.shape == (2, 8, 8, 16, 16) and c.dtype == torch.float32
    v = c.view(torch.float16).view(2, 8, 4, 2, 16, 32)                       # [n][y][K step][part][x][channel]
    hi_ref = torch.where(x.abs() < 6.103515625e-5, torch.zeros_like(x), x.half().float())
    assert float(v[1, 5, 2, 0, 7, 9]) == float(hi_ref[1, 5, 7, 64 + 9])
    assert float(v[1, 5, 2, 1, 7, 9]) == float(((x - hi_ref) * 2048.0).half()[1, 5, 7, 64 + 9])
    hi, lo = ops.unpack_split(c)
    assert torch.equal(hi.float(), hi_ref)
    back = hi.double() + lo.double() * 2.0 ** -11
    err = (back - x.double()).abs()
    assert bool((err <= x.double().abs() * 2.0 ** -22 + 1.5e-8).all())
    assert float(hi[0, 0, 0, 0]) == 0.0 and float(hi[0, 0, 0, 1]) == 0.0 and float(hi[0, 0, 0, 2]) != 0.0     # the normal-range rule
    hi2, lo2 = ops.unpack_split(ops.pack_split(back.float()))
    assert torch.equal(hi2.double() + lo2.double() * 2.0 ** -11, back)
