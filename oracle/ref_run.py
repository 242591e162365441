"""Runs the reference's own control logic on the CPU -- FIXTURE GENERATION ONLY.

``hbx_oracle.py`` restates the reference by hand.  This module runs the reference's programs
themselves, unmodified, so that their step-by-step outputs can be recorded
(tests/golden/make_ref_golden.py -> tests/golden/ref_*.npz) and the restatement and the HIP path
compared with those recordings.  It holds no text of the reference: the reference directory is
read at run time (argument, else the environment variable HBX_REFERENCE_DIR, else
/root/reference) and what is compiled from it lives in memory only.  Nothing marked ``gpu``,
``__graft_entry__.smoke()`` or ``bench.py`` may import this module; only the fixture generator and
the regeneration guard of tests/test_ref_parity_host.py do.

What makes the reference runnable without its dependencies (all absent here):

* ``sys.modules`` stand-ins for ``gymnasium`` (+ ``.spaces``), ``stable_baselines3`` (+ ``.common``,
  ``.common.callbacks``), ``torchvision`` and ``matplotlib`` (+ ``.pyplot``): do-nothing classes, the
  reference only subclasses or constructs them.
* ``torchOptics.optics`` / ``torchOptics.metrics``: ``Tensor``, ``simulate``, ``relativeLoss`` and
  ``get_PSNR`` on the oracle's float64 physics (transfer_function, mask_to_field, propagate,
  chan_stats, psnr_from_stats -- the path of ``Propagator.psnr``).  A recorded PSNR is therefore the
  oracle's number and any difference in a trace is control logic.  **The physics stays unpinned.**
* ``torch.Tensor.cuda``, ``torch.cuda.empty_cache`` and ``torch.cuda.synchronize`` are no-ops inside a
  ``Session`` and restored when it ends.

Two loaders: ``Session.load_module`` executes a whole file (env.py, env_md.py, env_group.py,
env_1024_24.py: they only define a class); ``Session.load_function`` picks one top-level function
out of a script by ``ast`` (the DBS*.py loops: the scripts' top level needs datasets and a GPU) and
compiles it into a namespace whose ``print``, ``os.makedirs`` and ``np.save`` go to a buffer and a
temporary directory.  A loaded module's ``IPS`` may be set (it passes a parameter); the reference's
text is never patched.
"""
from __future__ import annotations

import ast
import io
import os
import sys
import tempfile
import time
import types
from collections import defaultdict
from pathlib import Path
from typing import Callable, Optional

import numpy as np
import torch

from oracle import hbx_oracle as O

REF_ENV_VAR = "HBX_REFERENCE_DIR"
REF_DEFAULT = "/root/reference"


def reference_dir(path=None) -> Path:
    """The reference checkout: `path`, else $HBX_REFERENCE_DIR, else /root/reference."""
    p = Path(path or os.environ.get(REF_ENV_VAR) or REF_DEFAULT)
    if not (p / "env.py").is_file():
        raise FileNotFoundError(f"reference directory {p} not found (no env.py in it): pass its path or set "
                                f"{REF_ENV_VAR}")
    return p


def reference_available(path=None) -> bool:
    try:
        reference_dir(path)
        return True
    except FileNotFoundError:
        return False


class StopRun(Exception):
    """Raised from the PSNR hook to end a reference loop early (the regeneration guard's prefix)."""


class _Anything:
    """A do-nothing class: constructible with any arguments, subclassable."""

    def __init__(self, *args, **kwargs):
        pass


def _module(name: str, **attrs) -> types.ModuleType:
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


class Session:
    """Context manager: stand-ins installed, reference programs loadable, everything restored on exit.

    psnr_log collects every tt.relativeLoss(.., tm.get_PSNR) value in call order; on_psnr(k, value), if set,
    is called after the k-th (0-based) one is logged and may raise StopRun."""

    def __init__(self, ref_dir=None):
        self.ref = reference_dir(ref_dir)
        self.psnr_log: list = []
        self.on_psnr: Optional[Callable[[int, float], None]] = None
        self.saved_files: list = []
        self.out = io.StringIO()
        self._h = {}
        self._saved_modules = {}
        self._tmp = None

    # ---- the torchOptics stand-in, on the oracle's functions --------------------------------
    def _transfer(self, height, width, dx, dy, wl, z):
        key = (height, width, dx, dy, wl, z)
        if key not in self._h:
            self._h[key] = O.transfer_function(height, width, dx, dy, wl, z, O.TF_ASM)
        return self._h[key]

    def _tensor(self, data, meta=None):
        t = torch.as_tensor(data).detach()          # numpy input too (DBS_1024_24.py passes state slices)
        t.meta = dict(meta or {})
        return t

    def _simulate(self, field, z):
        meta = field.meta
        dx, dy = meta["dx"]
        wl = meta["wl"]
        if isinstance(wl, (tuple, list)):
            raise ValueError("stand-in tt.simulate: one wavelength per call")
        m = field.detach().numpy()
        h = self._transfer(m.shape[-2], m.shape[-1], float(dx), float(dy), float(wl), float(z))
        return torch.from_numpy(O.propagate(O.mask_to_field(m, O.FIELD_AMPLITUDE), h))

    @staticmethod
    def _get_psnr(x, y):
        return 10.0 * torch.log10(1.0 / torch.mean((x - y) ** 2))

    def _relative_loss(self, x, y, fn):
        xn = torch.as_tensor(x).detach().numpy().astype(np.float64)
        yn = torch.as_tensor(y).detach().numpy().astype(np.float64)
        if xn.shape != yn.shape or xn.ndim != 4 or xn.shape[0] != 1:
            raise ValueError(f"stand-in tt.relativeLoss: [1, G, H, W] pairs, got {xn.shape} / {yn.shape}")
        stats = np.stack([O.chan_stats(xn[0, g], yn[0, g]) for g in range(xn.shape[1])])
        if fn is self._get_psnr:
            value = O.psnr_from_stats(stats, xn[0].size, O.REL_LSQ, 1.0)
            self.psnr_log.append(value)
            if self.on_psnr is not None:
                self.on_psnr(len(self.psnr_log) - 1, value)
            return value
        sxy, sxx, _ = stats.sum(axis=0)
        return fn(torch.from_numpy(xn * (sxy / sxx)), torch.from_numpy(yn))

    # ---- install / restore -----------------------------------------------------------------
    def __enter__(self):
        self.tt = _module("torchOptics.optics", Tensor=self._tensor, simulate=self._simulate,
                          relativeLoss=self._relative_loss)
        self.tm = _module("torchOptics.metrics", get_PSNR=self._get_psnr)
        spaces = _module("gymnasium.spaces", **{n: type(n, (_Anything,), {}) for n in
                                                ("Dict", "Box", "Discrete", "MultiDiscrete")})
        callbacks = _module("stable_baselines3.common.callbacks", BaseCallback=type("BaseCallback", (_Anything,), {}),
                            CallbackList=type("CallbackList", (_Anything,), {}))
        common = _module("stable_baselines3.common", callbacks=callbacks)
        pyplot = _module("matplotlib.pyplot")
        stand_ins = {
            "gymnasium": _module("gymnasium", Env=type("Env", (_Anything,), {}), spaces=spaces),
            "gymnasium.spaces": spaces,
            "stable_baselines3": _module("stable_baselines3", PPO=type("PPO", (_Anything,), {}), common=common),
            "stable_baselines3.common": common,
            "stable_baselines3.common.callbacks": callbacks,
            "torchvision": _module("torchvision"),
            "matplotlib": _module("matplotlib", pyplot=pyplot),
            "matplotlib.pyplot": pyplot,
            "torchOptics": _module("torchOptics", optics=self.tt, metrics=self.tm),
            "torchOptics.optics": self.tt,
            "torchOptics.metrics": self.tm,
        }
        for name, mod in stand_ins.items():
            self._saved_modules[name] = sys.modules.get(name)
            sys.modules[name] = mod
        self._cuda, self._empty_cache, self._sync = torch.Tensor.cuda, torch.cuda.empty_cache, torch.cuda.synchronize
        torch.Tensor.cuda = lambda t, *a, **k: t
        torch.cuda.empty_cache = lambda: None
        torch.cuda.synchronize = lambda *a, **k: None       # env_1024_24.py's reset calls it
        self._tmp = tempfile.TemporaryDirectory(prefix="hbx_ref_run_")
        self._stdout = sys.stdout
        sys.stdout = self.out                       # the loaded modules' own prints
        return self

    def __exit__(self, *exc):
        sys.stdout = self._stdout
        torch.Tensor.cuda, torch.cuda.empty_cache, torch.cuda.synchronize = self._cuda, self._empty_cache, self._sync
        for name, mod in self._saved_modules.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod
        self._saved_modules.clear()
        self._tmp.cleanup()
        return False

    # ---- loaders ---------------------------------------------------------------------------
    def load_module(self, file_name: str, **set_attrs) -> types.ModuleType:
        """Executes a whole reference file as a module (never entered into sys.modules, no bytecode
        written); set_attrs (IPS=64) are assigned after it ran: its functions read them as globals."""
        path = self.ref / file_name
        mod = types.ModuleType("hbx_ref_" + path.stem)
        mod.__file__ = str(path)
        exec(compile(path.read_text(encoding="utf-8"), str(path), "exec"), mod.__dict__)
        for k, v in set_attrs.items():
            if k not in mod.__dict__:
                raise AttributeError(f"{file_name} has no module attribute {k}")
            setattr(mod, k, v)
        return mod

    def load_function(self, file_name: str, func_name: str) -> Callable:
        """One top-level function of a reference script, compiled alone into a namespace that holds
        the stand-ins; its prints go to self.out, os.makedirs and np.save into a temporary directory
        (np.save's relative path, shape and dtype are listed in self.saved_files)."""
        path = self.ref / file_name
        tree = ast.parse(path.read_text(encoding="utf-8"), filename=str(path))
        nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == func_name]
        if len(nodes) != 1:
            raise LookupError(f"{file_name}: {len(nodes)} top-level functions named {func_name}")
        root = Path(self._tmp.name)
        session = self

        class _Np:
            def __getattr__(self, name):
                return getattr(np, name)

            @staticmethod
            def save(file, arr, *a, **k):
                arr = np.asarray(arr)
                session.saved_files.append((str(file), arr.shape, str(arr.dtype)))
                target = root / str(file)
                target.parent.mkdir(parents=True, exist_ok=True)
                np.save(target, arr, *a, **k)

        class _Os:
            path = os.path

            @staticmethod
            def makedirs(name, *a, **k):
                (root / str(name)).mkdir(parents=True, exist_ok=True)

        ns = {"np": _Np(), "os": _Os(), "time": time, "torch": torch, "tt": self.tt, "tm": self.tm,
              "defaultdict": defaultdict, "print": lambda *a, **k: print(*a, **{**k, "file": self.out}),
              "__name__": "hbx_ref_" + path.stem}
        exec(compile(ast.Module(body=nodes, type_ignores=[]), str(path), "exec"), ns)
        return ns[func_name]

    # ---- helpers for the callers -----------------------------------------------------------
    def group_mean(self, state, lo, hi, wl, z=O.Z_DEFAULT):
        """mean_p |simulate(state[:, lo:hi])|^2 -> torch [1, 1, H, W], the way the reference writes it."""
        t = self._tensor(state[:, lo:hi], meta={"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wl})
        return torch.mean(self._simulate(t, z).abs() ** 2, dim=1, keepdim=True)


class Loader:
    """A DataLoader(batch_size=1) stand-in: iterating yields (target [1, G, H, W] tensor, [path])."""

    def __init__(self, targets, first_number: int = 801):
        self.targets = [np.asarray(t, np.float32) for t in targets]
        self.first_number = first_number

    def __iter__(self):
        for i, t in enumerate(self.targets):
            yield torch.from_numpy(t[None].copy()), [f"/data/valid/{self.first_number + i:04d}.png"]


def target_function_for(pairs):
    """The pre-model (BinaryNet) stand-in: maps each target of `pairs` = [(pre_model, target), ..] to
    its pre-model output [1, CH, H, W]."""
    table = {float(np.asarray(t).reshape(-1)[0]): np.asarray(p, np.float32) for p, t in pairs}

    def target_function(target):
        return torch.from_numpy(table[float(target.reshape(-1)[0])][None].copy())

    return target_function


class StandInEnv:
    """What the DBS*.py loop functions need of an env: reset() -> (obs, info) once (a second reset raises,
    which is how the loops' `while db_num <= max_datasets` ends), initial_psnr, trainloader.  The initial
    PSNR goes through the session's stand-in tt like every later one."""

    def __init__(self, session: Session, cfg: O.OpticsConfig, pre_model, target):
        self.session, self.cfg = session, cfg
        self.pre_model = np.asarray(pre_model, np.float32)[None].copy()
        self.target = np.asarray(target, np.float32).reshape(1, cfg.groups, cfg.height, cfg.width).copy()
        self.trainloader = Loader([self.target[0]])
        self.resets = 0
        self.initial_psnr = None
        self.state = None

    def reset(self):
        if self.resets:
            raise RuntimeError("stand-in env: one image only")
        self.resets += 1
        c, s = self.cfg, self.session
        self.state = (self.pre_model >= 0.5).astype(np.int8)
        self.initial_state = self.state.copy()
        means = [s.group_mean(self.state, g * c.planes, (g + 1) * c.planes, c.wavelengths[g], c.z)
                 for g in range(c.groups)]
        self.initial_psnr = s.tt.relativeLoss(torch.cat(means, dim=1), torch.from_numpy(self.target),
                                              s.tm.get_PSNR)
        s.psnr_log.clear()                          # the log then holds one PSNR per candidate
        obs = {"state": self.state, "state_record": np.zeros_like(self.state), "pre_model": self.pre_model,
               "recon_image": torch.cat(means, dim=1).numpy(), "target_image": self.target}
        return obs, {"state": self.state}
