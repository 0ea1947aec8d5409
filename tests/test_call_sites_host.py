"""CPU: every launch of a status-returning C-ABI entry point goes through `hip_ops._call` — named once, bound in
`_lib.SIGNATURES`, with the arity the header declares — and `_call` marshals and checks as the wrappers rely on."""
import ast
import re
from pathlib import Path

import pytest
import torch

from tests.test_layout import lib  # noqa: F401  (fixture: builds and loads libadvstep.so, which needs no GPU)

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "audio_deepfake_adversarial_attacks_amd"
MODULES = ("hip_ops.py", "lcnn_ops.py", "detector_ops.py", "frontend_ops.py", "datasets/wave_ops.py")


def launch_symbols():
    """Entry points that launch: declared `int advstep_x(..., advstep_stream_t stream)` in include/*.h."""
    header = "".join(h.read_text() for h in sorted((ROOT / "include").glob("*.h")))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"//[^\n]*", "", header)
    return set(re.findall(r"\bint\s+(advstep_[a-z0-9_]+)\s*\([^()]*\badvstep_stream_t\s+\w+\s*\)", header))


def test_every_launch_site_is_bound_and_has_the_right_arity():
    from audio_deepfake_adversarial_attacks_amd import _lib
    launches = launch_symbols()
    assert len(launches) >= 130 and launches <= set(_lib.SIGNATURES)
    for name in launches:                               # the helper appends the stream: it must be the last, pointer-sized slot
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.ctypes.c_int and argtypes[-1] is _lib.ctypes.c_void_p, name
    called, problems = set(), []
    for rel in MODULES:
        for node in ast.walk(ast.parse((PKG / rel).read_text())):
            if isinstance(node, ast.Attribute) and node.attr in launches:
                problems.append(f"{rel}:{node.lineno}: {node.attr} is called past _call")
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_call"):
                continue
            where = f"{rel}:{node.lineno}"
            first = node.args[0] if node.args else None
            if not (isinstance(first, ast.Constant) and isinstance(first.value, str)):
                if rel == "hip_ops.py" and isinstance(first, ast.Name) and first.id == "symbol":
                    continue                            # _call's own hand-over from its bracketed to its plain form
                problems.append(f"{where}: the symbol is not a string literal")
                continue
            symbol = first.value
            called.add(symbol)
            if symbol not in launches:
                problems.append(f"{where}: {symbol} is not a status-returning, stream-taking entry point")
            elif not any(isinstance(a, ast.Starred) for a in node.args):
                want = len(_lib.SIGNATURES[symbol][1]) - 1
                got = len(node.args) - 2                # past the symbol and the device
                if got != want:
                    problems.append(f"{where}: {symbol} takes {want} arguments before the stream, the call passes {got}")
            extra = {k.arg for k in node.keywords} - {"bracket", "work", "tensors"}
            if extra:
                problems.append(f"{where}: unknown keywords {sorted(extra)}")
    assert not problems, "\n".join(problems)
    assert len(called) >= 100                           # the walk did see the package's launch sites


def test_call_marshals_tensors_none_and_scalars_and_appends_the_stream(monkeypatch):
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    seen = []

    class _Lib:
        @staticmethod
        def advstep_fake_f32(*args):
            seen.append(args)
            return 0

    monkeypatch.setattr(hip_ops._lib, "load", lambda: _Lib)
    monkeypatch.setattr(hip_ops, "_stream", lambda device: 77)
    x, idx = torch.zeros(8), torch.zeros(3, dtype=torch.int32)
    assert hip_ops._call("advstep_fake_f32", torch.device("cpu"), x, None, idx[1:], 5, 0.25, bracket=None) is None
    (args,) = seen
    assert args == (x.data_ptr(), None, idx.data_ptr() + 4, 5, 0.25, 77)
    assert type(args[3]) is int and type(args[4]) is float


def test_call_raises_under_the_symbols_own_name(lib, monkeypatch):  # noqa: F811
    from audio_deepfake_adversarial_attacks_amd import _lib, hip_ops
    monkeypatch.setattr(hip_ops, "_stream", lambda device: None)
    x, out = torch.zeros(8), torch.zeros(8)
    # a null `grad`: rejected before any launch (test_layout.test_argument_validation_needs_no_device)
    with pytest.raises(_lib.AdvstepError, match=r"advstep_fgsm_step_f32: .*invalid argument"):
        hip_ops._call("advstep_fgsm_step_f32", torch.device("cpu"), x, None, out, 8, 0.1, 0.0, 1.0)
