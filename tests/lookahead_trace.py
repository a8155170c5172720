"""Which stream every launch of a sampler that generates ahead (prefetch_rng) lands on, without a GPU: stand-ins for
torch.cuda's streams and events and a wrapper around the NumPy kernel stand-ins log every public ops call as
"<stream> <name>" and every record / wait / synchronize with its stream and event.  Streams and events are numbered by first
appearance in the log; nothing else is normalised.  tests/test_lookahead_cpu.py compares the log of every case with
tests/golden/lookahead_trace.json (written from the package before the look-ahead generator got its one owner) and the
draws with those of a sampler that generates in line."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests.adapt_parity import perturbed_variances
from tests.fake_ops_chees import CheesFakeOps
from tests.fake_ops_mala_adapt import MalaAdaptFakeOps
from tests.mala_adapt_parity import eps_for, theta0

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookahead_trace.json")
C = 6


class FakeStream:
    cuda_stream = 0

    def __init__(self, rec):
        self._rec = rec

    def wait_event(self, ev):
        self._rec.log.append((self, "wait", ev))

    def synchronize(self):
        self._rec.log.append((self, "synchronize"))


class FakeEvent:
    def __init__(self, rec):
        self._rec = rec

    def record(self, stream=None):
        self._rec.log.append((stream if stream is not None else self._rec.current, "record", self))

    def synchronize(self):
        self._rec.log.append((self, "synchronize"))


class TracedOps:
    """Every public callable of `ops`, logged with the stream that is current when it is called (what the stand-in calls on
    itself is not: one entry per launch the sampler or the model asks for)."""

    def __init__(self, ops, rec):
        self._ops, self._rec = ops, rec

    def __getattr__(self, name):
        a = getattr(self._ops, name)
        if name.startswith("_") or not callable(a):
            return a

        def logged(*args, **kw):
            self._rec.log.append((self._rec.current, name))
            return a(*args, **kw)

        return logged


class Recorder:
    def __init__(self):
        self.log = []
        self.main = self.current = FakeStream(self)

    def install(self, monkeypatch):
        """Replace torch.cuda's Stream, Event, current_stream, stream and synchronize (monkeypatch: pytest's)."""
        @contextlib.contextmanager
        def stream(s):
            prev, self.current = self.current, s
            try:
                yield
            finally:
                self.current = prev

        monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: FakeStream(self))
        monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: FakeEvent(self))
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: self.current)
        monkeypatch.setattr(torch.cuda, "stream", stream)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: self.log.append(("device", "synchronize")))

    def mark(self, what):
        self.log.append(("--", what))

    def normalised(self):
        names = {}

        def name(x):
            if isinstance(x, (FakeStream, FakeEvent)):
                prefix = "s" if isinstance(x, FakeStream) else "e"
                return names.setdefault(x, prefix + str(sum(n[0] == prefix for n in names.values())))
            return x

        return [" ".join(name(x) for x in entry) for entry in self.log]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _lam(D):
    return np.logspace(0, 1, D)


def _hmc(D, path):
    def make(ops, prefetch):
        return bk.HMCDiag(bk.DiagGaussian(_lam(D), ops=ops), 0.05, 3, chains=C, seed=19, path=path, prefetch_rng=prefetch,
                          graph=False, ops=ops)
    return CheesFakeOps, make


def _mala(D, path):
    def make(ops, prefetch):
        return bk.MALA(bk.DiagGaussian(_lam(D), ops=ops), eps_for(D), init=theta0(C, D) / np.sqrt(_lam(D)), chains=C,
                       seed=19, path=path, prefetch_rng=prefetch, graph=False, ops=ops)
    return MalaAdaptFakeOps, make


SAMPLERS = {
    "HMCDiag auto D=8 (whole-draw kernel, momentum ahead in the state layout)": _hmc(8, "auto"),
    "HMCDiag auto D=40 (whole-draw kernel, chain-major normals, the generator's snapshot)": _hmc(40, "auto"),
    "HMCDiag opaque D=8 (step by step, kinetic energy ahead)": _hmc(8, "opaque"),
    "MALA D=8 (step by step)": _mala(8, "auto"),
    "MALA auto D=40 (two-pass, gradients recomputed in the step kernel)": _mala(40, "auto"),
    "MALA opaque D=40 (two-pass, model-opaque pair)": _mala(40, "opaque"),
}


def _precond(s):
    s.set_precond_diag(perturbed_variances(_lam(s._dim)))


def _assign(name, factor):
    return lambda s: setattr(s, name, factor * getattr(s, name))


_BOTH = {
    "rng_state()": lambda s: s.rng_state(),
    "state_dict()": lambda s: s.state_dict(),
    "load_state_dict(state_dict())": lambda s: s.load_state_dict(s.state_dict()),
    "set_precond_diag(v)": _precond,
    "warmup(12)": lambda s: s.warmup(12),
}
_HMC = {
    "warmup(12, adapt_trajectory=True)": lambda s: s.warmup(12, adapt_trajectory=True),
    "_stepsize assigned": _assign("_stepsize", 0.8),
}
_MALA = {
    "refresh_cache()": lambda s: s.refresh_cache(),
    "_epsilon assigned": _assign("_epsilon", 0.8),
}
# (a metric of the reference's kind excludes a preconditioner, which two of the operations above install: the assignment
# that makes the kinetic energy generated ahead stale is an operation of its own, on the step-by-step HMC case)
_METRIC = {"_metric assigned": lambda s: setattr(s, "_metric", np.linspace(0.5, 2.0, s._dim))}


def operations(sampler):
    if sampler.startswith("MALA"):
        return {**_BOTH, **_MALA}
    return {**_BOTH, **_HMC, **(_METRIC if "opaque" in sampler else {})}


CASES = [(s, op) for s in SAMPLERS for op in operations(s)]


def _snapshot(s, n):
    th, lp = [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(np.asarray(t).copy())
        lp.append(np.asarray(l).copy())
    return np.stack(th), np.stack(lp), s.rng_state().copy()


@functools.lru_cache(maxsize=None)
def run(sampler, op, prefetch):
    """Three draws, the operation, two more draws -> (the normalised log, [(theta, logp, rng_state) after the first draws,
    rng_state after the operation, (theta, logp, rng_state) after the last draws]).  Computed once per case."""
    rec = Recorder()
    with pytest.MonkeyPatch.context() as mp:
        rec.install(mp)
        ops_cls, make = SAMPLERS[sampler]
        s = make(TracedOps(ops_cls(), rec), prefetch)
        assert s._prefetch == prefetch
        rec.mark("three draws")
        before = _snapshot(s, 3)
        rec.mark(op)
        operations(sampler)[op](s)
        rec.mark("rng_state() after it")
        mid = s.rng_state().copy()
        rec.mark("two draws")
        after = _snapshot(s, 2)
        rec.mark("end")
        del s
    return rec.normalised(), [before, mid, after]


def key(sampler, op):
    return sampler + " | " + op


if __name__ == "__main__":  # PYTHONPATH=.:bayes-kit_amd python -m tests.lookahead_trace: write the golden file
    with open(GOLDEN, "w") as f:
        json.dump({key(s, op): run(s, op, True)[0] for s, op in CASES}, f, indent=0)
        f.write("\n")
