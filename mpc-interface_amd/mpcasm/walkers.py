"""Batched tick driver for a fleet of biped walkers.

The reference's walking loop (use_examples/simple_functional_example/
biped_mpc_loop.py:17-95) advances ONE walker: every tick it counts the step times
down, re-plans the step indicator matrix (tools.update_step_matrices -> plan_steps),
moves the stepping-area centres (tools.update_stepping_area) and re-assembles the QP,
whose width changes with the walking phase (34 / 36 unknowns at N=16).

Here a whole fleet advances in lock-step ticks, every walker with its own phase.
The QP *structure* depends only on the number ``p`` of steps inside the preview, so
the fleet is split into structure buckets (one compiled plan and one persistent
assembly launch per bucket and tick); what differs between walkers of a bucket is
numbers: the step indicator matrix ``E`` (a per-instance source), the stepping-area
centres (per-instance parameters) and the given vector.

:meth:`WalkerFleet.step` closes the loop on the device (biped_mpc_loop.py:50-95 for every walker):
assemble, solve to tolerance, and write each walker's next ``given`` from its solution
(:func:`biped_given_rules`, the reference's update_given_collector), with nothing read back.

``WalkerFleet(..., commands=True)`` steers the fleet: a device table of commands per walker (target velocity, where
to step) becomes, every tick and on the device, the parameters the reference's ``Formulation.update`` callbacks set
on the host (body.py:142-147, tools.update_stepping_area) -- :func:`biped_command_rules`, ``mpcasm_params_map``.
"""
import numpy as np

from . import problems
from .engine import checked_index  # noqa: F401  (the fleet's index of rows is checked where it is built)


def steps_in_preview(step_times, N):
    """Boolean mask of the step instants inside ``[0, N - 1)`` (tools.py:84 with count=0)."""
    return (step_times >= 0) & (step_times < N - 1)


def step_indicator(step_times, N):
    """``E[b, k, s] = 1`` when preview sample ``k`` lies after the ``s``-th step instant of
    walker ``b`` (tools.plan_steps, tools.py:79-101, for walkers that all have the same
    number of steps in the preview).  ``step_times``: ``(B, p)`` kept instants."""
    k = np.arange(N).reshape(1, N, 1)
    return (k > step_times[:, None, :]).astype(np.float64)


def stepping_centers(step_count, p, xy):
    """Alternating left/right centres of the next ``p`` stepping areas for every walker
    (tools.find_step_centers, tools.py:158-165): ``(B, p, 2)``."""
    side = (-1.0) ** (np.asarray(step_count) + 1)
    alt = np.tile([1.0, -1.0], p // 2 + 1)[:p]
    out = np.empty((len(side), p, 2))
    out[:, :, 0] = xy[0]
    out[:, :, 1] = side[:, None] * alt[None, :] * xy[1]
    return out


def biped_given_rules(form):
    """The reference's ``update_given_collector`` (biped_mpc_loop.py:81-92) as the rules of a given map
    (:meth:`mpcasm.engine.Assembler.given_map`): for every ``state, ID`` of the LIP,
    ``x0<axis>[ID] <- state[sample 0]``; for the states of the steps, ``s0<axis>[ID] <- state[sample 1]``
    (the support after the next sample); every bias column ``<- 0.0``."""
    rules = {}
    for dyn, prefix, sample in (("LIP", "x0", 0), ("steps", "s0", 1)):
        for state, ID in form.dynamics[dyn].state_ID.items():
            var = prefix + state[-2:]
            rule = rules.setdefault(var, [None] * len(form.given_ID[var]))
            rule[ID] = (state, sample)
    for var in form.dynamics["bias"].domain:
        rules[var] = 0.0
    return rules


# the commands of a walker on the biped formulation, in the order of the columns of WalkerFleet.commands
COMMAND_COLUMNS = ("vel_x", "vel_y", "step_x", "step_y")


def stepping_area_facets(form):
    """Indices (as in ``("limit", k, field)`` of a plan's ``param_slots``) of the facets of the biped's stepping
    area: it is the first box, so its facets are the first limits after the plain constraints."""
    first = sum(len(group) for group in form.constraints.values())
    return range(first, first + len(form.constraint_boxes["stepping area"].constraints))


def biped_command_rules(form):
    """What a walker's commands :data:`COMMAND_COLUMNS` set, as the rules of a parameter map
    (:meth:`mpcasm.engine.Assembler.param_map`) for ``form``, a biped formulation updated to its place in the step
    cycle: ``vel_x``, ``vel_y`` are the aims of the costs ``"track vel_x"``, ``"track vel_y"`` (the configuration's
    ``target_vel``); ``step_x``, ``step_y`` (its ``stepping_center``) place the centres of every facet of the
    ``"stepping area"`` box -- previewed step ``j``: ``center[j] = (step_x, sign * (+1, -1, +1, ...)[j] * step_y)``,
    which is tools.find_step_centers (tools.py:158-165) with the walker's ``side = (-1)^(step_count + 1)``
    supplied per instance as the launch's ``sign``."""
    rules = {("cost", "track vel_x", "aim"): ["vel_x"], ("cost", "track vel_y", "aim"): ["vel_y"]}
    box = form.constraint_boxes["stepping area"]
    for k, limit in zip(stepping_area_facets(form), box.constraints):
        p = np.atleast_2d(limit.center).shape[0]
        rules[("limit", k, "center")] = [
            ["step_x", {"column": "step_y", "signed": True, "c1": 1.0 if j % 2 == 0 else -1.0}] for j in range(p)]
    return rules


class FleetClock:
    """Vectorised step-time bookkeeping (biped_mpc_loop.py:41-45): every tick the step
    times count down; when the first reaches -1 they wrap by ``step_samples`` and the
    walker's step count goes up."""

    def __init__(self, step_samples, n_steps, phases):
        phases = np.asarray(phases, dtype=np.int64)
        base = np.array([(i + 1) * step_samples - 1 for i in range(n_steps)], dtype=np.int64)
        self.n = int(step_samples)
        self.step_times = base[None, :] - phases[:, None]
        self.step_count = np.zeros(len(phases), dtype=np.int64)

    def tick(self):
        self.step_times -= 1
        wrap = self.step_times[:, 0] == -1
        self.step_times[wrap] += self.n
        self.step_count[wrap] += 1


class WalkerFleet:
    """``batch`` walkers on the biped formulation of ``problems.biped``.

    ``phases[b]`` in ``[0, step_samples)`` is how many ticks walker ``b`` is ahead in its
    step cycle.  :meth:`tick` assembles the QPs of all walkers for the current tick and
    advances the clocks; it returns one entry per structure bucket:
    ``{"p": steps in preview, "index": walker ids, "P", "q", "G", "h": device tensors}``.

    :meth:`step` is one closed tick of the walking loop on :meth:`given_buffer` (assemble, solve,
    next ``given``) and :meth:`run` many of them.  ``on_unsolved`` is what happens to a walker whose QP
    is not solved -- the reference has no rule (``osqp_solve_qp`` returns None and its loop stops):
      * ``"hold"`` (default): only SOLVED and MAX_ITER solutions are applied; any other walker keeps its
        ``given`` for that tick and tries again at the next one, its clock advancing as ever;
      * ``"apply"``: every solution is applied except NON_CVX, whose iterates are NaN.
    ``polish``: :meth:`step` polishes every solved QP (:func:`mpcasm.engine.polish_qp`) between the solve and the
    next ``given``; off by default.
    ``warm``: :meth:`step` starts every solve from the walker's last solution moved one sample along
    (:func:`mpcasm.warm.shift_map`, :func:`mpcasm.engine.warm_start_qp`), with the step ``rho`` it ended with,
    where that solution was SOLVED; a walker whose last QP was not solved (or held), and every walker at its
    first tick, starts cold.  Off by default: a cold solve with OSQP's defaults every tick.
    ``commands``: the fleet can be steered.  :attr:`commands` is a device ``(batch, 4)`` float64 tensor in walker
    order, one row of :data:`COMMAND_COLUMNS` per walker, that starts from ``conf`` (``target_vel[0]``,
    ``target_vel[1]``, ``stepping_center[0]``, ``stepping_center[1]``); write it in place (or through
    :meth:`set_commands`) at any time.  Every :meth:`tick` and :meth:`step`, per bucket and ahead of its assembly,
    one :meth:`~mpcasm.engine.Assembler.apply_param_map` writes the walkers' commands into rows ``[:n]`` of the
    bucket's own ``asm.params`` (:func:`biped_command_rules`), on the device, and the assembly reads
    ``asm.params`` itself: no copy of the parameters is kept per place of the step cycle.  A captured graph holds
    that launch and the address of :attr:`commands`, so replays follow later edits.  In this mode ``asm.params``
    of each bucket is the authoritative tensor: an edit of a field that is not commanded, made on a bucket's
    assembler (``fleet.buckets[p]["asm"].set_param("cost", "minimize jerk", "weight", ...)``), holds from the next
    tick on, replays included (its rows are positions in the bucket's launch, not walkers: set such a field for
    all rows alike, or command it).  ``command_rules = (rules_for_form, columns)`` or ``(rules_for_form, columns,
    initial values)`` swaps in another map -- ``rules_for_form(form)`` returns a bucket's rules, for weights,
    margins or any other parameter; columns that are none of :data:`COMMAND_COLUMNS` start at the initial values
    (zero without).  Off by default: every walker keeps ``conf``'s gait and the parameters of a place are fixed
    the first time it comes round.
    ``soft``: soft limits (``engine.solve_qp(soft=...)``): a pair of scalars ``(lin, quad)`` makes every row of every
    QP soft -- a violation ``t > 0`` costs ``lin t + 1/2 quad t^2`` -- so that a disturbed walker still gets a plan
    instead of PRIMAL_INFEASIBLE; a callable gets a bucket's :class:`~mpcasm.engine.Assembler` and returns
    ``(lin, quad)``, scalars or ``(nc,)`` vectors (``asm.soft_rows({limit index: (lin, quad)})``; ``inf`` keeps a
    row hard).  The vectors are built once per bucket and passed at stride 0 on every tick, captured graphs
    included.  ``warm`` composes unchanged (the shifted start is only a start); with ``polish`` it is a
    ``ValueError`` (the polish models the hard problem).  None (default): hard limits, today's solve.
    """

    def __init__(self, batch, phases=None, conf=None, api=None, device=None, graphs=False, side_by_side=False,
                 on_unsolved="hold", polish=False, warm=False, commands=False, command_rules=None, soft=None):
        from .engine import Assembler, require_device
        from .solve_stage import stage_options

        stage_options(on_unsolved, polish, soft)
        self.on_unsolved = on_unsolved
        # what every bucket's solve stage (mpcasm.solve_stage) is built with, the first time the bucket steps.
        # polish=True: every solved QP is polished before its solution becomes the walker's next `given`;
        # soft=: the penalties of the solve, a pair or what makes one from a bucket's assembler
        self._stage_options = dict(on_unsolved=on_unsolved, polish=bool(polish), warm=bool(warm), soft=soft)
        # warm=True: one warm store for the fleet (a record per walker, sized by the widest bucket), built with
        # the first stage; per place of the step cycle the shift maps are kept with its other inputs
        self._warm, self._warm_store = bool(warm), None
        self._step_graphs = {}
        self._torch = require_device()
        self.conf = conf or problems.BipedConfig()
        self.api = api or problems.load_api("mpc_interface")
        self.batch = int(batch)
        n = self.conf.step_samples
        self.N = self.conf.horizon_lenght
        phases = np.arange(self.batch) % n if phases is None else np.asarray(phases)
        self.clock = FleetClock(n, self.conf.num_steps, phases)
        self.device = device
        self._ticks, self._cache = 0, {}
        # graphs=True: a tick's launches (parameter update, gather of `given`, one assembly per
        # structure bucket) are captured in a hipGraph the first time its place in the step cycle
        # comes round and replayed from then on -- the tick is a copy of `given` into a fixed
        # buffer and one graph launch instead of a dozen host-side calls
        self._use_graphs, self._graphs, self._given = bool(graphs), {}, None
        # side_by_side=True: inside the graph every bucket on a branch of its own with its share of the chip's
        # workgroup slots (capi.OPT_RESIDENT_GRID, by the number of its walkers).  Measured (round 4, 4 096
        # walkers: buckets of 512 and 3 584): 64 us per tick against 48 one after the other -- this runtime
        # replays a graph with parallel branches through signals between queues that cost more than the
        # second set-up they would hide; off by default
        self._side, self._side_by_side = [], bool(side_by_side)

        # one template formulation + assembler per structure bucket (steps in preview)
        self.buckets = {}
        for phi in range(n):
            times = np.array([(i + 1) * n - 1 - phi for i in range(self.conf.num_steps)])
            p = int(steps_in_preview(times, self.N).sum())
            if p in self.buckets:
                continue
            form = problems.biped(self.api, self.conf)
            form.update(step_times=times, step_count=0)
            asm = Assembler(form, batch=self.batch, device=device)
            torch = self._torch
            E = torch.zeros((self.batch, self.N, p, 1), dtype=torch.float64, device=asm.device)
            asm.bind_source(("steps", 0), E)
            # the stepping area is the first box: its facets are the first limits
            n_facets = len(form.constraint_boxes["stepping area"].constraints)
            first = sum(len(group) for group in form.constraints.values())
            facets = range(first, first + n_facets)
            # parameter columns of the centres of all facets of the stepping area, side by side
            cols = []
            for k in facets:
                sl, _ = asm.param_slice("limit", k, "center")
                cols.extend(range(sl.start, sl.stop))
            self.buckets[p] = dict(form=form, asm=asm, E=E, facets=facets,
                                   center_cols=torch.as_tensor(cols, dtype=torch.int64, device=asm.device))
        # commands=True: a parameter map per bucket and the fleet's command table, a row per walker
        self._commands = bool(commands) or command_rules is not None
        self.commands = self.command_columns = None
        if self._commands:
            rules_for, columns, initial = (tuple(command_rules) + (None,))[:3] if command_rules is not None \
                else (biped_command_rules, COMMAND_COLUMNS, None)
            columns = tuple(columns)
            for bucket in self.buckets.values():
                bucket["pmap"] = bucket["asm"].param_map(rules_for(bucket["form"]), columns)
            known = dict(zip(COMMAND_COLUMNS, (self.conf.target_vel[0], self.conf.target_vel[1],
                                               self.conf.stepping_center[0], self.conf.stepping_center[1])))
            row = np.array([float(known.get(c, 0.0)) for c in columns]) if initial is None \
                else np.asarray(initial, dtype=np.float64).reshape(len(columns))
            dev = next(iter(self.buckets.values()))["asm"].device
            self.command_columns = columns
            self.commands = self._torch.as_tensor(np.tile(row, (self.batch, 1)), device=dev).contiguous()

    @property
    def given_len(self):
        return next(iter(self.buckets.values()))["asm"].ng

    @property
    def warm_store(self):
        """The fleet's :class:`~mpcasm.engine.WarmStore` (a record per walker, in walker order); None for a
        fleet that is not warm, and before its first :meth:`step`."""
        return self._warm_store

    def set_commands(self, values, walkers=None):
        """Write :attr:`commands` in place without waiting for the device: ``values`` (tensor or array) is
        ``(batch, ncols)`` -- or ``(ncols,)``, the same for all -- or, with ``walkers`` (ids), one row per walker
        named.  The next tick reads them, a replayed graph included."""
        if not self._commands:
            raise ValueError("this fleet takes no commands (WalkerFleet(..., commands=True))")
        torch = self._torch
        cmd = self.commands
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values, dtype=np.float64))
        v = v.to(device=cmd.device, dtype=cmd.dtype, non_blocking=True)
        if walkers is None:
            cmd.copy_(v.expand_as(cmd))
        else:
            ids = np.asarray(walkers, dtype=np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= self.batch or np.unique(ids).size != ids.size):
                raise ValueError("walkers: distinct ids in [0, %d)" % self.batch)
            cmd.index_copy_(0, torch.as_tensor(ids, device=cmd.device), v.expand(ids.size, cmd.shape[1]))
        return cmd

    def structure_of(self):
        """Steps in the preview of every walker right now (its structure bucket)."""
        return steps_in_preview(self.clock.step_times, self.N).sum(axis=1)

    def _bucket_inputs(self):
        """This tick's per-bucket inputs on the device: walker ids, step indicator matrices,
        stepping-area centres.  The fleet advances in lock step, so they repeat with period
        ``2 * step_samples`` (the step cycle times the left/right alternation): each of those
        ticks is worked out once on the host (tools.plan_steps / find_step_centers semantics)
        and kept on the device in the shape the assembler takes as it is -- the indicator
        matrices as a full source tensor (bound per tick, no copy), the parameters with this place's
        centres of all facets in their columns (handed over per tick, no copy), the walkers' ids as the
        index of their rows of ``given``."""
        key = self._ticks % (2 * self.conf.step_samples)
        if key not in self._cache:
            torch = self._torch
            p_of = self.structure_of()
            entry = []
            for p, bucket in self.buckets.items():
                idx = np.nonzero(p_of == p)[0]
                if idx.size == 0:
                    continue
                if self._warm:     # (walkers that share the bucket of the tick before side by side)
                    idx, groups = self._shift_groups(p, idx)
                asm = bucket["asm"]
                dev = asm.device
                times = self.clock.step_times[idx]
                kept = times[steps_in_preview(times, self.N)].reshape(idx.size, p)
                E = torch.zeros((self.batch, self.N, p, 1), dtype=torch.float64, device=dev)
                E[:idx.size, :, :, 0] = torch.as_tensor(step_indicator(kept, self.N), device=dev)
                index = torch.as_tensor(checked_index(idx, self.batch), device=dev)
                if self._commands:
                    # a steered fleet keeps no parameters per place: the walkers' side (tools.find_step_centers:
                    # (-1)^(step_count + 1)), the sign of the tick's parameter map, is all the place adds
                    side = (-1.0) ** (self.clock.step_count[idx] + 1)
                    entry.append(dict(p=p, idx=idx, index=index, index_long=index.long(), E=E, params=None, key=key,
                                      sign=torch.as_tensor(side, dtype=torch.float64, device=dev)))
                else:
                    centers = stepping_centers(self.clock.step_count[idx], p, self.conf.stepping_center)
                    centers = torch.as_tensor(centers.reshape(idx.size, -1), device=dev)
                    # the bucket's parameters at this place of the cycle: the assembler's own, with the centres
                    # of the stepping area of these walkers in their columns -- a tensor per place, so that a
                    # tick copies nothing (only the centres change with the place in the cycle)
                    params = asm.params.clone()
                    params[:idx.size].index_copy_(1, bucket["center_cols"],
                                                  centers.repeat(1, len(bucket["facets"])))
                    entry.append(dict(p=p, idx=idx, index=index, index_long=index.long(), E=E, params=params,
                                      key=key))
                if self._warm:
                    entry[-1]["groups"] = [(a, b, torch.as_tensor(col, device=dev), torch.as_tensor(row, device=dev))
                                           for a, b, col, row in groups]
            self._cache[key] = entry
        return self._cache[key]

    def _shift_groups(self, p, idx):
        """The walkers ``idx`` of this place's bucket ``p``, reordered so that those that were in the same bucket
        a tick ago lie side by side, and per such group ``(first, last + 1, col_src, row_src)``: its positions
        in the bucket's launch and the shift maps from that bucket's form to this one's, built once on the host.
        A walker's first previewed step was taken in between exactly when its clock has just wrapped (its first
        step time is ``step_samples - 1`` again)."""
        from .warm import shift_map
        times = self.clock.step_times[idx]
        left = times[:, 0] == self.conf.step_samples - 1
        before = times + 1
        before[left] -= self.conf.step_samples
        p_before = steps_in_preview(before, self.N).sum(axis=1)
        keys = 2 * p_before + left
        order = np.argsort(keys, kind="stable")
        idx, keys = idx[order], keys[order]
        groups, new = [], self.buckets[p]
        for key in np.unique(keys):
            at = np.flatnonzero(keys == key)
            prev = self.buckets[int(key) // 2]
            col, row = shift_map(prev["form"], new["form"], bool(key % 2), horizon=self.N,
                                 prev_rows=[n for _, n in prev["asm"].plan.limit_rows],
                                 new_rows=[n for _, n in new["asm"].plan.limit_rows])
            groups.append((int(at[0]), int(at[-1]) + 1, col, row))
        return idx, groups

    def _launch(self, given, side_by_side=False, then=None):
        """This tick's launches for ``given`` (a device tensor): ONE assembly per structure bucket
        (its walkers' rows of ``given`` picked by index inside the kernel, the parameters of this place in
        the step cycle kept ready).  ``side_by_side``: every bucket on a stream of its own with its share
        of the workgroup slots (forked from and joined to the current stream: what a graph captures as
        parallel branches).  ``then(item, entry, stream)``: what follows a bucket's assembly on its stream."""
        from . import capi
        torch = self._torch
        items = self._bucket_inputs()
        side_by_side = side_by_side and len(items) > 1
        out = []
        if side_by_side:
            dev = self.buckets[items[0]["p"]]["asm"].device
            cur = torch.cuda.current_stream(dev)
            while len(self._side) < len(items) - 1:
                self._side.append(torch.cuda.Stream(device=dev))
            total = sum(item["idx"].size for item in items)
            slots = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
        for i, item in enumerate(items):
            p, idx = item["p"], item["idx"]
            bucket = self.buckets[p]
            asm = bucket["asm"]
            asm.bind_source(("steps", 0), item["E"])
            stream = None
            if side_by_side:
                asm.set_option(capi.OPT_RESIDENT_GRID, max(1, int(round(slots * idx.size / total))))
                if i:
                    stream = self._side[i - 1]
                    stream.wait_stream(cur)
            elif self._side:
                asm.set_option(capi.OPT_RESIDENT_GRID, -1)
            if self._commands:   # (the walkers' commands into the bucket's own parameters, ahead of the assembly)
                asm.apply_param_map(bucket["pmap"], self.commands, index=item["index"], sign=item["sign"],
                                    count=idx.size, stream=stream)
            # (no gather, no copy: the walkers' rows of `given` by index, the place's own parameters)
            P, q, G, h = asm.assemble(given, count=idx.size, index=item["index"], params=item["params"],
                                      stream=stream)
            out.append({"p": p, "index": idx, "P": P[:idx.size], "q": q[:idx.size],
                        "G": G[:idx.size], "h": h[:idx.size]})
            if then is not None:
                out[-1] = then(item, out[-1], stream)
        if side_by_side:
            for stream in self._side[:len(items) - 1]:
                cur.wait_stream(stream)
        return out

    def given_buffer(self):
        """The fleet's own ``(batch, ng)`` buffer of ``given`` on the device: a caller that writes the
        walkers' states straight into it and hands it to :meth:`tick` saves the copy a replayed graph needs
        (its launches read fixed addresses)."""
        if self._given is None:
            dev = next(iter(self.buckets.values()))["asm"].device
            self._given = self._torch.empty((self.batch, self.given_len), dtype=self._torch.float64, device=dev)
        return self._given

    def tick(self, given):
        """Assemble this tick's QPs (``given``: ``(batch, ng)`` tensor or array), then
        advance every walker's clock.  The results live in the assemblers' own buffers: they
        are valid until the next tick."""
        torch = self._torch
        dev = next(iter(self.buckets.values()))["asm"].device
        g = given if isinstance(given, torch.Tensor) else torch.as_tensor(
            np.asarray(given, dtype=np.float64), device=dev)
        g = g.to(dev)
        if not self._use_graphs:
            out = self._launch(g)
        else:
            if g is not self.given_buffer() and g.data_ptr() != self._given.data_ptr():
                self._given.copy_(g, non_blocking=True)
            key = self._ticks % (2 * self.conf.step_samples)
            if key not in self._graphs:
                self._launch(self._given)            # once as it is: kernels compiled, buffers there
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = self._launch(self._given, side_by_side=self._side_by_side)
                self._graphs[key] = (graph, out)
            graph, out = self._graphs[key]
            graph.replay()
        self.clock.tick()
        self._ticks += 1
        return out

    # ---- the closed loop ------------------------------------------------------------------
    def start_at_rest(self):
        """Every walker's row of :meth:`given_buffer` to the reference's start (biped_mpc_loop.py:26-33):
        the preview of zero ``given`` and ``optim`` -- all zeros -- with ``x0_y[0] = s0_y[0] = strt_y``."""
        form = next(iter(self.buckets.values()))["form"]
        row = np.zeros(self.given_len)
        for var in ("x0_y", "s0_y"):
            row[form.given_ID[var][0]] = self.conf.strt_y
        given = self.given_buffer()
        given.copy_(self._torch.as_tensor(row, device=given.device).expand_as(given))
        if self._warm_store is not None:      # (a warm fleet forgets its records: the first tick is cold)
            self._warm_store.reset()
        return given

    def _closed_bucket(self, item, entry, stream):
        """After a bucket's assembly, on its stream: the bucket's solve stage (:class:`mpcasm.solve_stage.SolveStage`,
        the narrow solver, made the first time the bucket steps; a warm fleet: one launch of the start per bucket
        of the tick before, the tag to expect the place before, the tag to store this place), then its walkers'
        next ``given`` from the solution, by the fleet's rule."""
        from .engine import WarmStore
        from .solve_stage import SolveStage

        bucket = self.buckets[item["p"]]
        asm, n = bucket["asm"], item["idx"].size
        stage = bucket.get("stage")
        if stage is None:   # (once per bucket, at fixed addresses for every place of the cycle and every graph)
            if self._warm and self._warm_store is None:
                self._warm_store = WarmStore(self.batch, max(b["asm"].no for b in self.buckets.values()),
                                             max(b["asm"].nc for b in self.buckets.values()), asm.device)
            stage = bucket["stage"] = SolveStage(asm, self.batch, store=self._warm_store, **self._stage_options)
            bucket["gmap"] = asm.given_map(biped_given_rules(bucket["form"]))
            if "soft" in stage.solver_kwargs:      # (the bucket's pair of rows, under the name it always had)
                bucket["soft"] = stage.solver_kwargs["soft"]
        out = stage.run(entry["P"], entry["q"], entry["G"], entry["h"], groups=item.get("groups", ()),
                        expect_tag=(item["key"] - 1) % (2 * self.conf.step_samples), tag=item["key"],
                        index=item["index"], count=n, stream=stream)
        asm.next_given(self.given_buffer(), out["x"], bucket["gmap"], index=item["index"], status=out["status"],
                       apply_mask=stage.apply_mask, count=n, stream=stream)
        return dict(out, p=item["p"], index=item["index"], index_long=item["index_long"])

    def step(self):
        """One closed tick of the walking loop on :meth:`given_buffer` (biped_mpc_loop.py:50-95 for every
        walker): per structure bucket, the assembly of :meth:`tick`, a cold :func:`~mpcasm.engine.solve_qp`
        with OSQP's defaults, and :meth:`~mpcasm.engine.Assembler.next_given` by the fleet's
        ``on_unsolved`` rule; then the clocks advance.  Nothing is read back: returns per bucket
        ``{"p", "index": walker ids, "x", "status", "iters"}`` (device tensors in the bucket's own buffers,
        valid until the next step; with ``polish`` also ``"polish"``, the verdicts of the polishing step; a warm
        fleet starts the solve from the store instead of cold and adds ``"warm"``, which walkers started warm).  With ``graphs``, each place of the step cycle runs its whole closed
        tick as one graph (captured the first time the place comes round, after running it as it is)."""
        torch = self._torch
        given = self.given_buffer()
        if not self._use_graphs:
            out = self._launch(given, then=self._closed_bucket)
        else:
            key = self._ticks % (2 * self.conf.step_samples)
            if key not in self._step_graphs:
                dev = given.device
                out = self._launch(given, side_by_side=self._side_by_side, then=self._closed_bucket)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):     # (captured, not run: this tick is done)
                    captured = self._launch(given, side_by_side=self._side_by_side, then=self._closed_bucket)
                self._step_graphs[key] = (graph, captured)
            else:
                graph, out = self._step_graphs[key]
                graph.replay()
        self.clock.tick()
        self._ticks += 1
        return [{k: v for k, v in entry.items() if k != "index_long"} for entry in out]

    def run(self, ticks, record=False):
        """:meth:`step` ``ticks`` times; returns device tensors ``status`` and ``iters`` ``(ticks, batch)``
        int32 in walker order and, with ``record``, ``given`` ``(ticks + 1, batch, ng)``: the fleet's
        ``given`` before the first tick and after every tick."""
        torch = self._torch
        given = self.given_buffer()
        i32 = dict(dtype=torch.int32, device=given.device)
        status = torch.zeros((ticks, self.batch), **i32)
        iters = torch.zeros((ticks, self.batch), **i32)
        trail = torch.empty((ticks + 1,) + tuple(given.shape), dtype=given.dtype, device=given.device) \
            if record else None
        if record:
            trail[0].copy_(given)
        for t in range(ticks):
            key = self._ticks % (2 * self.conf.step_samples)
            self.step()
            items = self._cache[key]
            for item in items:
                buf, n = self.buckets[item["p"]]["stage"].buffers, item["idx"].size
                status[t].index_copy_(0, item["index_long"], buf["status"][:n])
                iters[t].index_copy_(0, item["index_long"], buf["iters"][:n])
            if record:
                trail[t + 1].copy_(given)
        out = {"status": status, "iters": iters}
        if record:
            out["given"] = trail
        return out
