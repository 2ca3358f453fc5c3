"""What tests/test_bc_host.py and tests/test_bc_discrete_host.py share (no GPU): the kernel descriptors of
the built library, the source-text facts of a behaviour-cloning unit plus rocket_bc.inc, and the C ABI's
refusals and workspace sizes of the two calls, with the texts and numbers a build of the commit before the
fold returned."""
import ctypes
import os
import re
import subprocess
import tempfile

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
INC = os.path.join(CSRC, "rocket_bc.inc")


def kernel_descriptors():
    """{mangled name + '.kd': descriptor bytes} of every kernel in the built library"""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kd = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([B._llvm("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, B.OUT, os.path.join(d, "x")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for k, k0 in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % k), os.path.join(d, "b%d.co" % k)
            with open(part, "wb") as f:
                f.write(blob[k0:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.check_call([B._llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--%s" % B.ARCH, "--output=" + co])
            kd.update({n: v for n, v in B._elf_symbols(open(co, "rb").read()).items() if n.endswith(".kd")})
    return kd


def _includes(text):
    return re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M)


def check_unit(src, directory, after, discrete):
    """A behaviour-cloning unit: alone in csrc/<directory>, compiled in the linking step after `after` with
    the learner's settings; the prefetch define ahead of the policy include; the kernels are rocket_bc.inc's,
    included once after the unit's `#define RR_BC_DISCRETE <discrete>`, and that text includes the learner's
    bodies (no copies) and holds both gradient-tower instantiations."""
    assert os.path.dirname(src) == os.path.join(CSRC, directory) and os.path.isfile(src)
    assert os.listdir(os.path.dirname(src)) == [os.path.basename(src)]
    assert src in B.sources() and INC in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    assert len(cmds) == 6  # five compile steps and the link
    mine = [c for c in cmds if src in c]
    assert mine == [cmds[-1]] and "-shared" in mine[0]  # compiled in the linking step, a module of its own
    assert mine[0].index(after) < mine[0].index(src) < mine[0].index(B.SRC_COLLECT_STATS)
    assert mine[0][-1] == B.SRC_COLLECT_STATS and not any(INC in c for c in cmds)
    for flag in B.COLLECT_FLAGS:  # the learner's code-generation setting
        assert flag in mine[0]
    assert not any(f in mine[0] for f in B.EXACT_FLAGS if f != "-mllvm")
    unit, inc = open(src).read(), open(INC).read()
    assert unit.index("#define RR_POL_PREFETCH_A 1") < unit.index('#include "rocket_policy.inc"')
    assert _includes(unit) == ["rocket_device.h", "rocket_policy.inc", "rocket_ppo.inc", "rocket_bc.inc"]
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+RR_BC_DISCRETE[ \t]+(\S+)", unit, flags=re.M)
    assert defines == [str(discrete)]
    assert unit.index("#define RR_BC_DISCRETE") < unit.index('#include "rocket_bc.inc"')
    assert "__global__" not in unit  # no kernel of its own
    # the learner's bodies, not copies of them
    assert _includes(inc) == ["rocket_ppo_finish_body.inc", "rocket_ppo_adam_body.inc"]
    assert "ppo_grad_tower<OBS, ACT, 0, false, false, 1>" in inc and "ppo_grad_tower<OBS, ACT, 0, false, false, 3>" in inc
    assert inc.count("__global__") == 4 and "__builtin_amdgcn_mfma" not in inc + unit
    for name in _includes(unit) + _includes(inc):
        assert os.path.join(CSRC, name) in B.sources() and not name.endswith(".hip"), name


# bytes for batch 2, 128, 129, 4097, 65 536
BATCHES = (2, 128, 129, 4097, 65536)
WORKSPACE_BYTES = {
    ("rr_bc_update", 14, 3): (102592, 102592, 128240, 923328, 3359888),
    ("rr_bc_update", 7, 2): (98736, 98736, 124128, 911280, 3323520),
    ("rr_bc_update_discrete", 7, 2): (101360, 101360, 127264, 930288, 3391168),
    ("rr_bc_update_discrete", 7, 3): (101360, 101360, 127264, 930288, 3391168),
    ("rr_bc_update_discrete", 7, 4): (101360, 101360, 127264, 930288, 3391168),
}


def check_workspace_sizes(call):
    lib = _lib.load()
    n = ctypes.c_int64()
    shapes = [k[1:] for k in WORKSPACE_BYTES if k[0] == call]
    assert len(shapes) == (3 if "discrete" in call else 2)
    for shape in shapes:
        for bs, want in zip(BATCHES, WORKSPACE_BYTES[(call,) + shape]):
            assert getattr(lib, call + "_workspace_size")(*shape, bs, ctypes.byref(n)) == _lib.RR_OK
            assert n.value == want, (call, shape, bs)


GAUSS_SHAPE = "supported (obs_dim, act_dim) are (14, 3) and (7, 2)"
CAT_OBS, CAT_K = "obs_dim must be 7 (the 3DOF env)", "n_choices must be in 2 .. 4"


def _ptrs(k, null_at=None):
    arr = (ctypes.c_void_p * k)(*[0x100000 + 0x1000 * i for i in range(k)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def check_refusals(call, shape, n_tensors, bad_shapes):
    """Never-read fake device addresses and a NULL stream: every refusal of `call` and of its
    *_workspace_size returns RR_EINVAL before a launch, with exactly the text the build before the fold
    gave. bad_shapes: ((obs_dim, act_dim or n_choices), text) pairs."""
    lib = _lib.load()
    V = ctypes.c_void_p
    fn, size_fn, sz = getattr(lib, call), getattr(lib, call + "_workspace_size"), call + "_workspace_size"
    p, nbytes = V(0x70000), ctypes.c_int64()

    def refused(rc, who, text):
        assert rc == _lib.RR_EINVAL, (who, text, rc)
        assert lib.rr_last_error() == ("%s: %s" % (who, text)).encode(), (lib.rr_last_error(), who, text)

    for bad, text in bad_shapes:
        refused(size_fn(*bad, 64, ctypes.byref(nbytes)), sz, text)
    for bs in (1, 0, -5):
        refused(size_fn(*shape, bs, ctypes.byref(nbytes)), sz, "batch >= 2 and bytes required")
    refused(size_fn(*shape, 64, None), sz, "batch >= 2 and bytes required")
    assert size_fn(*shape, 4096, ctypes.byref(nbytes)) == _lib.RR_OK
    need = nbytes.value
    names = ("params", "grads", "m", "v", "step")

    def run(shape=shape, obs=p, acts=p, idx=p, batch=4096, ent=1e-3, l2=0.0, lr=p, stats=p, flags=0, ws=V(0x200000),
            ws_bytes=need, **lists):
        ls = [lists.get(k, _ptrs(n_tensors)) for k in names]
        return fn(*shape, *ls, obs, acts, idx, batch, ent, l2, lr, 0.9, 0.999, 1e-8, stats, flags, ws, ws_bytes, None)

    for bad, text in bad_shapes:
        refused(run(shape=bad), call, text)
    for bs in (1, 0, -5):
        refused(run(batch=bs), call, "batch >= 2 required")
    for name in names + ("obs", "acts", "idx", "lr", "ws"):
        refused(run(**{name: None}), call, "null argument")
    for name in names:
        for hole in (0, 7, 8, 9, 10, 11, n_tensors - 1):
            refused(run(**{name: _ptrs(n_tensors, null_at=hole)}), call,
                    "null parameter, gradient or optimizer-state tensor")
    refused(run(ws_bytes=need - 16), call, "workspace smaller than %s" % sz)
    refused(run(batch=8192), call, "workspace smaller than %s" % sz)  # sized for 4096 rows: 32 workgroups, not 64
    refused(run(ws=V(0x200008)), call, "workspace must be 16-B aligned")
    for bad in (float("nan"), -0.1, -float("inf")):
        refused(run(ent=bad), call, "ent_weight must be >= 0")
        refused(run(l2=bad), call, "l2_weight must be >= 0")
    for flags in (0x2, 0x4, 0x80000001):
        refused(run(flags=flags), call, "unknown flag bits")
    for stats in (p, None):  # the statistics are optional: refused for the flag, not for them
        refused(run(stats=stats, flags=0x2), call, "unknown flag bits")
