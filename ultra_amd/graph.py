"""hipGraph capture of the engine's steps.

The forward of one batch is ~30 short launches (layer-0 kernels, 5 rspmm + updates on the entity graph, 5 fused
relation-graph layers, prologue, projections, readout); on a static graph with a fixed batch shape
the launch sequence never changes, so it is captured once into a HIP graph (torch.cuda.CUDAGraph drives
hipStreamBeginCapture / hipGraphLaunch) and replayed: one host call per forward instead of ~30.  Our kernels are enqueued on
torch's current stream, which is the capturing stream during capture; plans, schedules and the
LDS opt-in are created by the eager warm-up runs, so nothing allocates inside the captured region.

Four steps are replayed this way -- the bare forward (GraphedForward), a batch of the filtered-ranking protocol
(GraphedEvalStep), a batch of top-k answers (predict._GraphedPredictStep) and the training step (train.GraphedTrainStep) -- and
all four inherit ONE lifecycle, `Capture`: warm-up on a side stream, pinning, capture, release.  What a captured graph points
at stays alive and in place for as long as its Capture does:
  * the aggregation plans its warm-up runs asked for (rspmm.record_plans) are held and pinned (ultra_plan_pin) -- the
    plan cache is an LRU and would otherwise free device arrays the graph still reads once enough other graphs have
    been seen; plans the capture never used stay free to grow their scratch buffers.  A warm-up or capture that fails
    (out of memory, models.NotOnFusedPath, a kernel error) unpins them at once and leaves no graph behind: __del__ of a
    half-built object is not something to rely on;
  * the model's parameters are watched (param_state): the forward caches stacked copies of some weights (relation
    projections), so a parameter update (optimizer step, load_state_dict) makes the next call re-capture instead of
    replaying stale values.
"""
import contextlib

import torch

from . import rspmm


def param_state(model):
    """What a capture that reads the model's parameters remembers of them: it is stale once this changes."""
    return tuple((p.data_ptr(), p._version) for p in model.parameters())


class Capture(object):
    """warm_up(step, runs), then capture(step) once or twice; release() lets go of the plans and the graphs.

    plans: the plans the warm-up asked for, each pinned once; graphs: the captured graphs, in order; stream: the warm-up's
    side stream.  no_grad: warm-up and capture run under torch.no_grad() (the inference steps; the training step not)."""

    def __init__(self, device, no_grad=True):
        self.device, self.no_grad = device, no_grad
        self.plans, self.graphs, self.stream = [], [], None

    @property
    def graph(self):
        return self.graphs[0]

    _pinned = property(lambda self: self.plans)       # (the list's former, private name: still readable)

    @property
    def exact_order(self):
        """Every plan this capture uses is a reference-order plan (what it really uses, not the default kind)."""
        return all(plan.exact for plan in self.plans)

    def release(self):
        while self.plans:
            self.plans.pop().pin(-1)
        self.graphs = []

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _grad_mode(self):
        return torch.no_grad() if self.no_grad else contextlib.nullcontext()

    @contextlib.contextmanager
    def recording(self):
        """The plans get_plan() hands out inside the block are pinned when it ends, exactly those and each once (what the
        Capture held before is released first); an exception inside leaves nothing pinned."""
        self.release()
        try:
            with rspmm.record_plans() as used:
                yield
            for plan in used.plans:
                plan.pin(+1)
                self.plans.append(plan)
        except BaseException:
            self.release()
            raise

    def warm_up(self, step, runs):
        """`runs` eager step() on a fresh side stream that waits for the current one; joined and synchronised afterwards."""
        with torch.cuda.device(self.device), self.recording():
            self.stream = torch.cuda.Stream()
            self.stream.wait_stream(torch.cuda.current_stream())
            with self._grad_mode(), torch.cuda.stream(self.stream):
                for _ in range(runs):
                    step()
            torch.cuda.current_stream().wait_stream(self.stream)
            torch.cuda.synchronize()

    def capture(self, step, stream=None, pool=None, upload=False):
        """step() recorded into a new graph (appended to `graphs`); returns what step() returned.  stream: the capture stream
        (None: torch's own); pool: the memory pool of an earlier graph to share; upload: replay once and synchronise -- the first
        launch of an instantiated graph also uploads it (kernel arguments, node descriptors), and that is then part of building
        the graph, not of the caller's first batch (a real step for a graph that updates state: not for those)."""
        try:
            with torch.cuda.device(self.device):
                graph = torch.cuda.CUDAGraph()
                # thread-local capture mode: helper threads of the process (RCCL's watchdog polls events) must not be able to
                # invalidate the capture; everything captured here is enqueued by this thread
                with self._grad_mode(), torch.cuda.graph(graph, pool=pool, stream=stream, capture_error_mode="thread_local"):
                    out = step()
                if upload:
                    graph.replay()
                    torch.cuda.synchronize()
        except BaseException:
            self.release()
            raise
        self.graphs.append(graph)
        return out


class GraphedForward(Capture):
    """score = GraphedForward(model, data, example_batch)(batch) for batches of example_batch's shape."""

    def __init__(self, model, data, example_batch, warmup=3, launch_grid=0):
        """launch_grid > 0: the aggregation kernels of this capture are launched with that many workgroups instead of one per
        CU (rspmm.tuning_scope(grid=...) around warm-up and capture) -- see PipelinedForward."""
        assert example_batch.is_cuda, "graph capture needs GPU tensors"
        Capture.__init__(self, example_batch.device)
        self.model = model
        self.data = data
        self.warmup = warmup
        self.launch_grid = int(launch_grid)
        self.static_batch = example_batch.clone()
        self._recapture()

    def _recapture(self):
        model, data = self.model, self.data
        self._watched = None                  # (a capture that fails is made again by the next call)
        model.eval()

        def forward():
            return model(data, self.static_batch)
        with rspmm.tuning_scope(**({"grid": self.launch_grid} if self.launch_grid > 0 else {})):
            self.warm_up(forward, self.warmup)
            # (a table of cached relation representations the capture reads from stays alive with the capture)
            self._rel_table_ref = getattr(model, "_rel_table", None)
            self.static_out = self.capture(forward, upload=True)
        self.valid = getattr(model.entity_model, "_pending_valid", None) if hasattr(model, "entity_model") else None
        self._watched = param_state(model)

    def _load_input(self, batch):
        """batch -> the graph's input buffer.  A plain 16-byte streaming kernel: the runtime's device-to-device memcpy
        costs ~9 us for these 2.8 MB, a third of it launch overhead of its generic copy kernel."""
        nbytes = batch.numel() * batch.element_size()
        if batch.is_cuda and batch.is_contiguous() and batch.dtype == self.static_batch.dtype and nbytes % 16 == 0 \
                and batch.data_ptr() % 16 == 0 and self.static_batch.data_ptr() % 16 == 0:
            from ._lib import check, lib, stream_of
            check(lib.ultra_stream_copy(self.static_batch.data_ptr(), batch.data_ptr(), nbytes, stream_of(batch)))
        else:
            self.static_batch.copy_(batch, non_blocking=True)

    def __call__(self, batch, check=False):
        if batch.shape != self.static_batch.shape:
            raise ValueError("GraphedForward was captured for batch shape %s, got %s"
                             % (tuple(self.static_batch.shape), tuple(batch.shape)))
        if param_state(self.model) != self._watched:      # weights changed since the capture: the cached stacks are stale
            self._recapture()
        self._load_input(batch)
        self.graph.replay()
        if check and self.valid is not None:
            assert bool(self.valid.all()), "every row of `batch` must share its head (or tail) and its relation (models.py:196-197)"
        return self.static_out


def slot_stream(device, priority=0):
    """A stream for one pipeline slot (PipelinedForward, evaluate()'s two captured steps)."""
    with torch.cuda.device(device):
        return torch.cuda.Stream(priority=priority)


def _skip_streams(device, priority):
    """(measurements: ULTRA_SLOT_STREAM_SKIP=n takes n streams of that priority from torch's pool first -- the runtime maps streams
    onto hardware queues in creation order, so this shifts which queues the slots' streams land on)"""
    import os
    for _ in range(int(os.environ.get("ULTRA_SLOT_STREAM_SKIP", "0"))):
        st = slot_stream(device, priority)
        with torch.cuda.stream(st):
            torch.zeros(1, device=device)
        st.synchronize()


def pick_slot_streams(device, n, trial, n_cand=None):
    """The streams the pipeline slots run on, chosen by MEASUREMENT.  The HIP runtime maps a process's streams onto a small pool
    of hardware queues (GPU_MAX_HW_QUEUES of them) as they are created, and how the slots' launches interleave depends on which
    queues their streams land on -- i.e. on how many streams of which priority the process made before (torch's side streams, the
    capture streams, RCCL's).  Measured on MI355X, bench.py --steps 20 --warmup 5, ms per step first run / repeats
    (profiles/r5_slot_streams.txt, r5_experiments.txt):

        plain process, two slots:   normal-priority pair 0.573 / 0.562 - 0.567, high 0.573 / 0.567 - 0.573 in one call -- 0.577 / 0.679
                                    (trial) in another; the pair made after THREE other streams of its level: normal 0.606 / 0.597 - 0.612,
                                    high 0.764 / 0.757
        plain process, three slots: 0.595 / 0.580 - 0.594 (normal, first streams), 0.568 / 0.566 - 0.570 (normal, after three others),
                                    0.569 / 0.558 - 0.573 (high, first), 0.645 / 0.637 - 0.652 (high, after two others)
        a launcher's rank (RCCL):   two slots 0.616 / 0.587 - 0.605 (normal), 0.584 / 0.573 - 0.576 (high); three slots on the high
                                    pair 0.565 - 0.588 / 0.555 - 0.572

    The same step runs between 0.557 and 0.764 ms depending on nothing but where its streams landed, no level or position is right
    everywhere, and nothing the process can ask the runtime says which is.  So the pipeline tries a handful of candidate sets when
    it is built -- alternately normal- and high-priority, each made of fresh streams (which also moves the next candidate to other
    queues) -- times a few steps on each (`trial(streams)` -> seconds per step, the step's post-op included; ~ 25 ms a candidate) and
    keeps the fastest.  ULTRA_SLOT_STREAM_CANDIDATES sets how many (12); ULTRA_SLOT_STREAM_PRIORITY=0 / -1 pins the first set of that
    level (measurements).  Returns (streams, report)."""
    import os
    forced = os.environ.get("ULTRA_SLOT_STREAM_PRIORITY")
    if forced not in (None, "", "auto"):
        prio = int(forced)
        _skip_streams(device, prio)
        return [slot_stream(device, prio) for _ in range(n)], {"chosen": "high" if prio < 0 else "normal", "forced": True}
    n_cand = max(2, int(os.environ.get("ULTRA_SLOT_STREAM_CANDIDATES", "12")) if n_cand is None else int(n_cand))
    best, report = None, []
    for k in range(n_cand):
        prio = 0 if k % 2 == 0 else -1
        streams = [slot_stream(device, prio) for _ in range(n)]
        trial(streams)                                   # (first use of a stream: queue creation, not timed)
        t = min(trial(streams) for _ in range(2))
        report.append(["normal" if prio == 0 else "high", round(1e3 * t, 4)])
        if best is None or t < best[0]:
            best = (t, k, streams)
    return best[2], {"chosen": report[best[1]][0], "candidate": best[1], "forced": False, "trial_ms": report}


def shared_launch_grid(device):
    """Workgroups of an aggregation launch that leaves a quarter of the chip to the other batch in flight (whole XCD-sized
    multiples: 192 of 256 -- 200 and 208 measured 4 % slower than either neighbour)."""
    import os
    if os.environ.get("ULTRA_SHARED_GRID"):      # (measurements: tools/step_probe.py sweeps it)
        return int(os.environ["ULTRA_SHARED_GRID"])
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max((3 * cus // 4) // 64 * 64, 3 * cus // 4 if cus < 86 else 64)


class PipelinedForward(object):
    """`depth` captured forwards (own input, activation and output buffers each) replayed round-robin on `depth` streams:
    consecutive batches are independent, so the launches of one batch that leave the chip idle (relation model, glue) run
    beside the entity layers of its neighbour -- 0.69 -> 0.62 ms per batch at the benchmark point with two in flight.

    share_chip (True; "auto", the default: where the layers' activations fit the last-level cache): the aggregation kernels of each
    capture are launched with three quarters of the chip's CUs as workgroups instead of one per CU.  A reference-order
    workgroup owns its CU (160 KB of LDS), so behind a full-size launch nothing else starts; at 192 of 256 the entity layers of
    the batches in flight still follow one another, but the other batch's short, latency-bound launches (relation-graph layers,
    layer 0, projections, readout) find 64 free CUs at any time.  tools/share_probe.py, twelve runs of 20 steps, ms per batch
    (median; first run): 256 workgroups 0.614; 0.641 -- 224: 0.616; 0.635 -- 192: 0.603; 0.627 -- 128: 0.599; 0.610, but there
    two entity layers run side by side (199 us each against 152 alone on half a chip) and how the two streams' phases fall decides
    between 0.60 and 0.65 (bench.py's repeats alternated between the two).  The sums do not depend on the split: the schedule
    only decides WHICH workgroup walks a row, never the order inside it.

    Reference-order plans only: the re-associating plans keep per-plan scratch that concurrent forwards would share."""

    def __init__(self, model, data, example_batch, depth=2, warmup=3, slot_factory=None, share_chip="auto", trial_post=None):
        """slot_factory: what builds one slot's forward (default: a GraphedForward of `model`); a CPU batch gets slots without
        streams -- the collective-ordering contract of `post=` is testable without a GPU (tests/test_distributed.py).
        trial_post: the `post=` the caller will pass to every step (a multi-GPU step's all-gather): the short trial that picks the
        slots' streams (pick_slot_streams) then runs the steps WITH it -- how a pair of streams interleaves depends on the
        collective's stream too (measured: a launcher's rank whose trial left the all-gather out could not tell the pairs apart,
        0.593 vs 0.590 ms, and then ran at 0.60 on the pair that runs at 0.574 with the other).  Every rank runs the same number of
        trial steps, so the collectives pair up."""
        if not rspmm._plan_defaults["exact_order"]:
            raise RuntimeError("PipelinedForward needs the reference-order plans (the re-associating plans own scratch buffers)")
        grid = 0
        if share_chip == "auto":
            # measured with half-chip launches (tools/step_probe.py, two in flight, ms per batch, shared / whole-chip): FB15k237
            # shape 0.592 / 0.623, WN18RR 0.795 / 0.781, CoDEx-L 1.967 / 1.905 -- it pays where a layer's input and output of all
            # samples stay in the last-level cache (60 MB at the first, 167 and 319 MB at the others)
            share_chip = example_batch.is_cuda and data is not None and \
                2 * example_batch.shape[0] * int(data.num_nodes) * 256 <= 128 << 20
        if share_chip and int(depth) > 1 and example_batch.is_cuda:
            grid = shared_launch_grid(example_batch.device)
        self.launch_grid = grid
        make = slot_factory or (lambda: GraphedForward(model, data, example_batch, warmup=warmup, launch_grid=grid))
        self.slots = []
        for _ in range(int(depth)):
            self.slots.append(make())
            if not getattr(self.slots[-1], "exact_order", True):     # (what the capture really uses, not the default kind)
                raise RuntimeError("PipelinedForward: this model's forward uses a re-associating plan (scratch buffers that "
                                   "concurrent forwards would share); run its batches one at a time")
        dev = example_batch.device
        self.device = dev
        self.calls = 0
        self.stream_report = None
        if dev.type == "cuda" and len(self.slots) > 1:
            def trial(streams, steps=12):
                import time
                self.streams = streams
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    self(example_batch, post=trial_post)
                self.join()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) / steps
            self._trial = trial
            self.streams, self.stream_report = pick_slot_streams(dev, len(self.slots), trial)
            self.calls = 0
        elif dev.type == "cuda":
            self.streams = [slot_stream(dev)]
        else:
            self.streams = [None for _ in self.slots]

    def __call__(self, batch, post=None):
        """Enqueue the forward of `batch` on the next slot's stream; post(score), if given, runs on that stream right behind
        it (e.g. the all-gather of a multi-GPU step) and its result is returned instead."""
        k = self.calls % len(self.slots)
        self.calls += 1
        stream = self.streams[k]
        if stream is None:      # (CPU slots: the call order IS the program order)
            out = self.slots[k](batch)
            return post(out) if post is not None else out
        stream.wait_stream(torch.cuda.current_stream(self.device))     # `batch` was produced on the caller's stream ...
        if batch.is_cuda:
            batch.record_stream(stream)                                 # ... and may be released by the caller right after this call
        with torch.cuda.stream(stream):
            out = self.slots[k](batch)
            if post is not None:
                out = post(out)
        return out

    def join(self):
        if self.device.type != "cuda":
            return
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    def settle(self, step_fn, steps=48, tolerance=0.03, collective=False):
        """The pipeline's warm-up, watched: run step_fn(0 .. steps - 1) (each enqueues one step through this pipeline), and if they
        took more than `tolerance` over the trial's winning figure per step -- the ~ 25 ms trial that chose the slots' streams can
        be wrong about the steady state: the same streams were seen at 0.57 and 0.97 ms per step within one process
        (profiles/r5_slot_streams.txt) -- choose the streams ONCE more (replays onto another stream set cost nothing), time
        `steps` steps on the new set and keep whichever set was faster.  collective: the steps contain a collective (a multi-GPU
        step's all-gather) -- every rank then takes the same decision (any rank slow -> all re-pick: their trial steps pair up).
        Returns the report (also merged into self.stream_report); a pipeline without a choice to make just runs the steps."""
        import time

        def timed():
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for i in range(steps):
                step_fn(i)
            self.join()
            torch.cuda.synchronize(self.device)
            return (time.perf_counter() - t0) / max(steps, 1)
        report = self.stream_report
        if (self.device.type != "cuda" or len(self.slots) < 2 or not report or report.get("forced") or not report.get("trial_ms")
                or steps < 8):
            for i in range(steps):
                step_fn(i)
            return None
        first = timed()
        best_trial = min(ms for _, ms in report["trial_ms"]) * 1e-3
        slow = first > (1.0 + tolerance) * best_trial
        if collective and torch.distributed.is_available() and torch.distributed.is_initialized():
            flag = torch.tensor([1.0 if slow else 0.0], device=self.device)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
            slow = bool(flag.item() > 0)
        out = {"settle_steps": steps, "settled_ms": round(1e3 * first, 4), "trial_best_ms": round(1e3 * best_trial, 4), "repicked": False}
        if slow:
            old = self.streams
            self.streams, again = pick_slot_streams(self.device, len(self.slots), self._trial)
            self.calls = 0
            second = timed()
            out.update(repicked=True, repick_trial_ms=again.get("trial_ms"), repick_settled_ms=round(1e3 * second, 4))
            keep_old = second > first
            if collective and torch.distributed.is_available() and torch.distributed.is_initialized():
                # (one decision for the job: the sets are kept or swapped back on every rank alike -- a rank's streams only matter
                # to its own clock, but the ranks' steps must stay paired)
                flag = torch.tensor([1.0 if keep_old else 0.0], device=self.device)
                torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                keep_old = bool(flag.item() > 0)
            if keep_old:
                self.streams = old
            out["kept"] = "first choice" if keep_old else "second choice"
        self.stream_report = dict(report, settle=out)
        return out


class GraphedEvalStep(Capture):
    """One batch of the filtered-ranking protocol (script/run.py:131-160) as ONE hipGraph replay: candidate construction
    (tasks.all_negative), the tail and the head forward, and the two fused rank kernels.  Per batch the host copies three
    small tensors into the graph's inputs -- the (bs, 3) triples and the two (bs + 1) offset vectors into the known-answer
    lists, which evaluate() builds once for its whole shard -- and replays; the (2 bs, 3) rows [rank, #negatives, is_tail]
    come back in a static buffer.  No (bs, N, 3) candidate copy, no score clone, no per-batch sort / unique."""

    def __init__(self, model, data, batch_size, known_tail, known_head, warmup=2):
        from . import tasks
        from ._lib import check, lib, stream_of
        dev = data.edge_index.device
        Capture.__init__(self, dev)
        self.model, self.data, self.bs = model, data, batch_size
        self.t_index, self.h_index = known_tail.contiguous(), known_head.contiguous()
        self.batch = torch.zeros(batch_size, 3, dtype=torch.long, device=dev)
        self.t_ptr = torch.zeros(batch_size + 1, dtype=torch.long, device=dev)
        self.h_ptr = torch.zeros(batch_size + 1, dtype=torch.long, device=dev)
        self.rows = torch.zeros(2 * batch_size, 3, dtype=torch.long, device=dev)
        self.rows[:batch_size, 2] = 1
        n = data.num_nodes

        def step():
            t_batch, h_batch = tasks.all_negative(data, self.batch)
            stream = stream_of(dev)
            for cand, pos_col, ptr, index, lo in ((t_batch, 1, self.t_ptr, self.t_index, 0),
                                                   (h_batch, 0, self.h_ptr, self.h_index, batch_size)):
                pred = model(data, cand).float().contiguous()
                pos = self.batch[:, pos_col].contiguous()
                rank = torch.empty(batch_size, dtype=torch.long, device=dev)
                neg = torch.empty_like(rank)
                check(lib.ultra_filtered_rank(pred.data_ptr(), pos.data_ptr(), ptr.data_ptr(), index.data_ptr(), batch_size, n,
                                              rank.data_ptr(), neg.data_ptr(), stream))
                self.rows[lo:lo + batch_size, 0] = rank
                self.rows[lo:lo + batch_size, 1] = neg

        # (a capture that fails -- out of memory for the second step of evaluate(), a kernel error -- leaves no plan pinned)
        self.warm_up(step, warmup)
        self.capture(step)

    def __call__(self, batch, t_ptr, h_ptr):
        """rows (2 bs, 3) of this batch -- a view of the static buffer: copy before the next call."""
        self.batch.copy_(batch, non_blocking=True)
        self.t_ptr.copy_(t_ptr, non_blocking=True)
        self.h_ptr.copy_(h_ptr, non_blocking=True)
        self.graph.replay()
        return self.rows
