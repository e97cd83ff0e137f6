"""Deferred completion of a training step's solves: the step-count policy (`Deferred`), the loop that repeats a missed
batch (`DeferredLoop`), the per-function tokens of their keys.  `integrate._HipOdeint` asks `Deferred.active` what to enqueue."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import weakref
from typing import Dict, List, Optional

import torch

from . import _lib


class Deferred:
    """Deferred completion of the solves of a training step: keep the queue fed across the solver.

    A dopri5 solve normally ends with one read-back of the device controller (did the steps enqueued finish the
    interval?), and the host dispatches everything behind it only afterwards -- the GPU idles while PyTorch launches
    the head, and again while it launches the stem's backward.  With deferred completion enabled, a solve whose step
    count is known from the previous iteration enqueues exactly that many steps and returns at once; whether they
    were the steps needed is written by the device into a record, and a MISS (the interval unfinished after them, or an
    error status; finishing EARLY is no miss -- the steps past the end return at once) bumps the device flag
    `miss_flag`.  The output of a missed solve is its y0 (the trajectory buffer is pre-filled), and every number
    computed from it -- loss, accuracy -- belongs to a step whose update was skipped: `step_verdicts()` lists which.  Nothing that commits results may run unconditionally:
    `optim.FusedSGD.skip_flag = deferred.miss_flag` predicates the parameter update on the device, so a step with a
    miss changes nothing (under data parallelism the flag rides in the reducer's last bucket, so every rank skips
    together).  The host looks at a record one iteration later, when it is long complete: the true step count in it
    becomes the next guess; a miss makes the next solve of that kind run with a read-back again.  While a solve's
    count is still moving one spare step is enqueued, so only a count that jumps by two or more is a miss.

        deferred = integrate.Deferred(device)        # opt-in; the drop-in API is unaffected while none is active
        opt.use_deferred(deferred)                   # FusedSGD: the update is predicated on the flag and zeroes it
        with deferred:                               # (nothing runs blind in a scope no optimizer was armed with)
            for x, y in loader:
                loss = F.cross_entropy(model(x), y); loss.backward(); opt.step(); opt.zero_grad()
        deferred.resolve()                           # -> number of steps whose update was skipped

    `func.nfe` advances by the predicted count at once and is corrected when the record is read (sums over an
    epoch are exact); `last_*_stats` of a deferred solve hold the prediction."""

    active = None      # the instance whose `with` block is open
    # How many steps to enqueue for a solve whose true count nobody knows yet.  A step past the end of the interval returns
    # at its first instruction in every kernel, but its ~40 launches still cost ~0.1 ms; a miss costs the iteration and
    # (DeferredLoop) the repetition of two batches: ~150x more.  So: enqueue the LARGEST count of the last HIST solves of
    # this kind (a count that wobbles by one between iterations then wastes half a step on average; a count that DROPS is
    # followed after HIST iterations), plus ONE spare step whenever a larger count is not unlikely:
    #   * the history is short (CALM);
    #   * the last solve overshot the end of its interval by less than FRAGILE of its last step (the record carries the
    #     last step: node_step_record.t_prev / dt_used) -- step sizes that come out a few percent smaller on the next batch
    #     then need one step more;
    #   * a count above everything in the history was seen within the last QUIET solves.
    # Margins: FRAGILE 0.15 / QUIET 16 in round 4; the measured sweep on the cfg-3 bench loop (profiles/r04_deferred_policy_cfg3.txt)
    # has 0.05 / 8 at +1.3 % images/s with 0 misses in 200 steps, soaked again in round 5 (profiles/r05_deferred_soak_cfg3.txt).
    # Round 3 enqueued last count + 1 until eight exact predictions in a row -- at tol 1e-5 that never happened, and every
    # solve carried one or two dead steps (profiles/r03_r_cfg3_steps.txt: 29 dead component GEMMs per step).
    HIST = int(os.environ.get('NODE_DEFERRED_HIST', 8))
    CALM = 4
    FRAGILE = float(os.environ.get('NODE_DEFERRED_FRAGILE', 0.05))      # (environment: A/B measurements, tools/deferred_soak.py)
    QUIET = int(os.environ.get('NODE_DEFERRED_QUIET', 8))

    def __init__(self, device):
        self.device = torch.device(device)
        self.miss_flag = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.guess: Dict[tuple, Optional[int]] = {}
        self.calm: Dict[tuple, int] = {}          # solves of a key since its history was last reset
        self.hist: Dict[tuple, List[int]] = {}    # true step counts of the last HIST solves of a key
        self.fragile: Dict[tuple, bool] = {}      # the last solve of a key barely reached the end of its interval
        self.quiet: Dict[tuple, int] = {}         # solves of a key since one needed more steps than any in its history
        self.pending: Dict[tuple, tuple] = {}
        self._seq: Dict[tuple, int] = {}
        self.records: Dict[tuple, tuple] = {}
        self.misses = 0
        self.blind_solves = 0
        self.dead_steps = 0        # steps enqueued past the end of their interval (read from the records)
        self.verdicts: List[tuple] = []   # (blind solve index, key kind, missed?) in the order the records were read
        self.armed = False         # set by FusedSGD.use_deferred: without a predicated commit point nothing runs blind
        self._last_enqueued: Dict[tuple, int] = {}

    def __enter__(self):
        Deferred.active = self
        return self

    def __exit__(self, *exc):
        Deferred.active = None
        return False

    def _buffers(self, key):
        b = self.records.get(key)
        if b is None:
            n = C.sizeof(_lib.NodeStepRecord)
            b = (torch.zeros(n, dtype=torch.uint8, device=self.device), torch.zeros(n, dtype=torch.uint8).pin_memory(),
                 torch.cuda.Event())
            self.records[key] = b
        return b

    def plan(self, key, func=None):
        """Steps to enqueue blind for `key`, or None for a solve with a read-back.  Looks first at the record the
        previous blind solve of this key left (one iteration old: complete): its true step count becomes the new
        guess (and corrects `func.nfe`, which was advanced by the guess), a miss sends the next solve back to a
        read-back.  While a key's count is still moving, ONE spare step is enqueued (a step past the end of the
        interval returns at once on the device: ~0.1 ms of launches) so that a count that grows by one is no miss."""
        pend = self.pending.pop(key, None)
        if pend is not None:
            guessed, fref, enqueued = pend
            if func is None and fref is not None:
                func = fref()
            dev, host, event = self._buffers(key)
            event.synchronize()
            r = _lib.NodeStepRecord.from_buffer_copy(bytes(host.numpy().tobytes()))
            self.verdicts.append((self._seq.pop(key, -1), key[0], bool(r.miss)))
            if len(self.verdicts) > 4096:
                del self.verdicts[:2048]
            if r.miss:
                self.misses += 1
                self.guess[key] = None
                self.calm[key] = 0
                self.hist[key] = []
            else:
                if func is not None and r.steps != guessed:
                    func.nfe = getattr(func, 'nfe', 0) + 6 * (r.steps - guessed)    # late, but sums stay exact
                self.dead_steps += max(0, enqueued - int(r.steps))
                # solver time runs upwards in both directions (a solve towards smaller t integrates -t): how far past the
                # end of the interval did the last step land, in units of that step?
                end = key[-1][-1] if key[0] == 'fwd' else -key[-1][0]
                self.fragile[key] = bool(r.dt_used > 0.0 and (r.t - end) < self.FRAGILE * r.dt_used)
                self._observe(key, int(r.steps))
        g = self.guess.get(key)
        if not g or not self.armed:
            return None
        return g, self._enqueue(key)

    def _observe(self, key, steps):
        h = self.hist.setdefault(key, [])
        self.quiet[key] = 0 if (h and int(steps) > max(h)) else self.quiet.get(key, self.QUIET) + 1
        h.append(int(steps))
        del h[:-self.HIST]
        self.calm[key] = self.calm.get(key, 0) + 1
        self.guess[key] = int(steps)

    def _spare(self, key):
        """One spare step while a count above the history's maximum is not unlikely (see the class constants)."""
        h = self.hist.get(key) or []
        return len(h) < self.CALM or self.fragile.get(key, False) or self.quiet.get(key, self.QUIET) < self.QUIET

    def _enqueue(self, key):
        h = self.hist.get(key) or [self.guess[key]]
        return max(h) + (1 if self._spare(key) else 0)

    def blind_args(self, key, enqueue):
        dev, _, _ = self._buffers(key)
        self._last_enqueued[key] = int(enqueue)
        return (enqueue, dev, self.miss_flag)

    def launched(self, key, guessed, func=None):
        dev, host, event = self._buffers(key)
        host.copy_(dev, non_blocking=True)
        event.record(torch.cuda.current_stream(self.device))
        self.pending[key] = (guessed, weakref.ref(func) if func is not None else None, self._last_enqueued.pop(key, guessed))
        self._seq[key] = self.blind_solves
        self.blind_solves += 1

    def learned(self, key, steps):
        """A solve of `key` ran with a read-back: its count starts a new history."""
        self.hist[key] = []
        self.calm[key] = 0
        self.fragile[key] = False
        self.quiet[key] = 0
        self._observe(key, int(steps))

    def forget(self):
        """Drop every step-count guess (the next solve of each kind runs with a read-back and learns its count anew)."""
        for k in list(self.guess):
            self.guess[k] = None
            self.calm[k] = 0
            self.hist[k] = []

    def force_counts(self, counts):
        """Tests: pretend every kind of solve (or those in the {key: n} mapping) has needed exactly n steps for a long
        time -- the next blind solve enqueues n steps and no spare one."""
        for k in list(self.guess):
            n = counts.get(k) if isinstance(counts, dict) else counts
            if n is None:
                continue
            self.guess[k] = int(n)
            self.hist[k] = [int(n)] * self.CALM
            self.calm[k] = self.CALM
            self.fragile[k] = False
            self.quiet[k] = self.QUIET

    def step_verdicts(self):
        """[(blind solve index, 'fwd' | 'bwd', missed)] for the records read so far (one iteration late): a caller that
        logs losses or drives an LR schedule from them drops the iterations whose solves missed."""
        return list(self.verdicts)

    def settled(self):
        """True once every kind of solve seen so far runs blind with exactly its last count (no spare step, no larger count
        in the history window):
        from then on a training step enqueues no launch that returns at once."""
        return bool(self.guess) and all(g and not self._spare(k) and max(self.hist[k]) == self.hist[k][-1]
                                        for k, g in self.guess.items())

    def resolve(self):
        """Wait for every outstanding record (a synchronisation point) and count the misses."""
        for key in list(self.pending):
            self.plan(key)
        return self.misses


class DeferredLoop:
    """Training steps under deferred completion that never lose an update: a miss costs time, not training data.

    `Deferred` alone SKIPS the optimizer step of an iteration one of whose solves missed.  Here the device flag is
    STICKY -- nothing zeroes it behind the optimizer step, so once a solve has missed, that update and every later one
    is skipped on the device -- and the host keeps each batch until its verdict is in.  `lag` iterations later (the copy
    of the flag as the optimizer step saw it is long complete by then: no stall) the host reads the verdict; on a miss
    it drains the queue, zeroes the flag, forgets the step-count guesses, and runs the voided batches again IN ORDER
    with a read-back per solve, each under the random-generator state its first attempt started from.  The sequence
    of committed updates is therefore exactly the synchronous run's (tests/test_gpu_deferred.py: parameters
    bit-identical after a forced miss).  Under data parallelism the flag every rank reads is the all-reduced one
    (`dp.GradientReducer.carry_flag`), so all ranks void and repeat the same batches together.

        loop = integrate.DeferredLoop(deferred, opt, step_fn, reducer)     # step_fn(*batch) -> anything
        for x, y in loader:
            for result in loop.step(x, y):      # results of batches whose update is now known to be committed
                log(result)
        for result in loop.flush(): log(result)
    """

    def __init__(self, deferred: 'Deferred', opt, step_fn, reducer=None, lag: int = 1):
        self.d, self.opt, self.step_fn, self.lag = deferred, opt, step_fn, max(0, int(lag))
        opt.use_deferred(deferred, reducer)
        opt.flags_to_reset = []            # sticky: only the host clears the flag, after it has seen the miss
        self.queue: List[list] = []        # [batch, result, rng state, pinned flag copy, event]
        self.retries = 0                   # batches run a second time
        self.miss_events = 0
        self.steps = 0
        self._pool: List[tuple] = []       # (pinned float, event) pairs of settled entries, reused

    def _rng(self):
        return torch.cuda.get_rng_state(self.d.device), torch.get_rng_state()

    def _set_rng(self, st):
        torch.cuda.set_rng_state(st[0], self.d.device)
        torch.set_rng_state(st[1])

    def _run(self, batch):
        with self.d:
            return self.step_fn(*batch)

    def _settle(self, keep: int):
        """Pop committed entries until `keep` remain; on a miss repeat everything queued.  Returns committed results."""
        out = []
        while len(self.queue) > keep:
            batch, result, rng, host, event = self.queue[0]
            event.synchronize()
            if float(host[0]) == 0.0:
                self.queue.pop(0)
                self._pool.append((host, event))
                out.append(result)
                continue
            # a solve of this iteration (on some rank) missed: its update and every later one were skipped on the device
            self.miss_events += 1
            torch.cuda.synchronize(self.d.device)
            self.d.resolve()
            self.d.miss_flag.zero_()
            self.d.forget()
            voided, self.queue = self.queue, []
            flag, self.opt.skip_flag = self.opt.skip_flag, None
            armed, self.d.armed = self.d.armed, False
            try:
                for b, _, r, _, _ in voided:
                    self._set_rng(r)      # the generator state the first attempt started from: after the last repeat
                    out.append(self._run(b))   # it stands where the synchronous run's stands
                    self.retries += 1
            finally:
                self.opt.skip_flag = flag
                self.d.armed = armed
        return out

    def step(self, *batch):
        done = self._settle(self.lag)
        rng = self._rng()
        result = self._run(batch)
        host, event = self._pool.pop() if self._pool else (torch.zeros(1, dtype=torch.float32).pin_memory(), torch.cuda.Event())
        src = self.opt.skip_flag if self.opt.skip_flag is not None else self.d.miss_flag
        host.copy_(src, non_blocking=True)      # the flag as this iteration's optimizer step saw it
        event.record(torch.cuda.current_stream(self.d.device))
        self.queue.append([batch, result, rng, host, event])
        self.steps += 1
        return done

    def flush(self):
        return self._settle(0)


_TOKENS = itertools.count(1)
_TOKEN_OF: 'weakref.WeakKeyDictionary' = weakref.WeakKeyDictionary()


def _func_token(func):
    """A key for `func` that is never reused and never shared: id() can be handed to a new object after the old one
    was collected (a new dynamics function would inherit a stale step-count guess), and an attribute on the module
    would travel with `copy.deepcopy(model)` (an EMA / evaluation copy would share its original's pending record).
    Tokens therefore live in a weak-keyed table beside the modules, not on them."""
    try:
        tok = _TOKEN_OF.get(func)
        if tok is None:
            tok = _TOKEN_OF[func] = next(_TOKENS)
        return tok
    except TypeError:          # not weak-referenceable / unhashable: fall back to identity
        return id(func)
