"""Fixer — WW-style fixing of nonants whose x-bar has converged, with the
bookkeeping on the device (mirrors ``mpisppy/extensions/fixer.py:20-329``; same
options, tuples, warnings, errors and progress lines).

The reference's ``miditer`` loops over every local scenario and fixer tuple in
Python, reads x-bar and x-squared-bar through Pyomo, and calls ``xvar.fix`` plus
the persistent solver's ``update_var`` per scenario.  Here the convergence
counts, the fixed flags and the fixed values live on the device per (node,
slot) entry of the x-bar vector:

  _update_fix_counts (:114-129),
  the decisions of iterk (:226-304)
  and of iter0 (:131-223)            phx_fixer_step: one launch over the [NNS]
                                     entries, the number of new fixes copied to
                                     a pinned host word
  xvar.fix / update_var              only when that number is nonzero:
                                     SPOpt._fix_where_device (one read-back of
                                     the flags, phx_fix_nonants_where)

While every local scenario has the same slots fixed (always, on a two-stage
tree) the following solves run on the library's fixed-subset lane module;
problems served by the workgroup or sparse solvers (sslp, netdes) solve on the
generic path once something is fixed.

Differences from the reference, on purpose:
  * ``Fixer_tuple``'s first element identifies the variable as rho_setter lists
    do here: ``id(var)`` of a variable of the scenario's model, or the
    ``varid`` of a nonant view (``s._mpisppy_data.nonant_indices``) when the
    scenarios come from a batch creator and have no model.
  * The reference tests ``xb - xvar.lb`` per scenario and then raises
    "Variation in fixing across scenarios detected".  Here the bounds are per
    entry, taken from the node's scenarios when the tables are built; a column
    with an lb or ub lag whose bounds differ within its node raises ValueError
    there.
  * The counters count unique (node, slot) entries; on a two-stage tree that is
    the reference's raw count divided by the number of local scenarios.
  * While the Fixer runs it owns the fixedness of the nonants: what it has not
    fixed is free after each of its fixes.
"""
import numpy as np
import torch

from .extension import Extension

_HOW = {1: "nb", 2: "lb", 3: "ub"}


def _name(xvar):
    return getattr(xvar, "name", str(xvar))


def Fixer_tuple(xvar, th=None, nb=None, lb=None, ub=None):
    """ Somewhat self-documenting way to make a fixer tuple.
    Args:
        xvar: the nonant variable (a model variable or a nonant view)
        th (float): compared to sqrt(abs(xbar_sqared - xsquared_bar))
        nb: (int) None means ignore; for iter k, number of iters
                  converged anywhere.
        lb: (int) None means ignore; for iter k, number of iters
                  converged within th of xvar lower bound.
        ub: (int) None means ignore; for iter k, number of iters
                  converged within th of xvar upper bound

    Returns:
        tuple: a tuple to be appended to the iter0 or iterk list of tuples
    """
    if th is None and nb is None and lb is None and ub is None:
        print("warning: Fixer_tuple called for Var=", _name(xvar),
              "but no arguments were given")
    if th is None:
        th = 0
    if nb is not None and lb is not None and nb < lb:
        print("warning: Fixer_tuple called for Var=", _name(xvar),
              "with nb < lb, which means lb will be ignored.")
    if nb is not None and ub is not None and nb < ub:
        print("warning: Fixer_tuple called for Var=", _name(xvar),
              "with nb < ub, which means ub will be ignored.")
    varid = getattr(xvar, "varid", None)
    return (id(xvar) if varid is None else varid, th, nb, lb, ub)


class Fixer(Extension):

    def __init__(self, ph):
        super().__init__(ph)
        self.ph = ph
        self.cylinder_rank = self.ph.cylinder_rank
        self.options = ph.options
        self.fixeroptions = self.options["fixeroptions"]  # required
        self.verbose = self.options["verbose"] or self.fixeroptions["verbose"]
        # this function is scenario specific (takes a scenario as an arg)
        self.id_fix_list_fct = self.fixeroptions["id_fix_list_fct"]
        self.dprogress = ph.options["display_progress"]
        self.fixed_prior_iter0 = 0
        self.fixed_so_far = 0
        self.boundtol = self.fixeroptions["boundtol"]
        # (PH iteration, node-slot entry, 1 nb / 2 lb / 3 ub, value) of every fix
        self.events = []

    # ------------------------------------------------------------ tables
    def populate(self, local_scenarios):
        """The per-entry tables of both rules from every local scenario's
        tuples (fixer.py:66-102), made identical on every rank and uploaded."""
        ph = self.ph
        NNS = int(ph.NNS)
        self.local_scenarios = local_scenarios
        self.iter0_fixer_tuples = {}
        self.fixer_tuples = {}
        self.threshold = {}
        self.iter0_threshold = {}
        self._no_iter0 = None
        self._no_iterk = None
        ABSENT = -np.inf
        # rows: th, nb, lb lag, ub lag -- for iter0, then for iterk
        tab = np.full((8, max(NNS, 1)), ABSENT)
        idx = ph._xbar_idx
        for k, (sname, s) in enumerate(local_scenarios.items()):
            target = ph._models[sname] if ph._models is not None else s
            t0, tk = self.id_fix_list_fct(target)
            self.iter0_fixer_tuples[sname], self.fixer_tuples[sname] = t0, tk
            if t0 is None and self._no_iter0 is None:
                self._no_iter0 = sname
            if tk is None and self._no_iterk is None:
                self._no_iterk = sname
            for tuples, thr, base, what in ((t0, self.iter0_threshold, 0, "iter0 fixer threshold across scenarios."),
                                            (tk, self.threshold, 4, "fixer threshold across scenarios")):
                if tuples is None:
                    continue
                for (varid, th, nb, lb, ub) in tuples:
                    try:
                        ndn_i = s._mpisppy_data.varid_to_nonant_index[varid]
                    except Exception:
                        print("Are you trying to fix a Var that is not nonant?")
                        raise
                    if ndn_i not in thr:
                        thr[ndn_i] = th
                    elif th != thr[ndn_i]:
                        print(sname, ndn_i[0], ndn_i[1], th)
                        raise RuntimeError("Attempt to vary " + what)
                    e = int(idx[s._slot_of_key(ndn_i), k])
                    tab[base:base + 4, e] = [th, -1 if nb is None else nb, -1 if lb is None else lb,
                                             -1 if ub is None else ub]
        # the column bounds per entry over the node's scenarios: [max lb, -min lb, max ub, -min ub]
        b = ph.batch
        N, S = idx.shape
        bnd = np.full((4, max(NNS, 1)), ABSENT)
        if N and S:
            cols = np.asarray(b.nonant.slot_col, dtype=np.int64)
            lbm = np.broadcast_to(b.lb[:, cols].T if b.bnd_vary else b.lb[cols][:, None], (N, S))
            ubm = np.broadcast_to(b.ub[:, cols].T if b.bnd_vary else b.ub[cols][:, None], (N, S))
            for row, a in enumerate((lbm, -lbm, ubm, -ubm)):
                np.maximum.at(bnd[row], idx.ravel(), a.ravel())
        allv = ph.mpicomm.allreduce_np(np.concatenate([tab, bnd]), op="max")
        tab, bnd = allv[:8], allv[8:]
        lags = tab[[1, 2, 3, 5, 6, 7]]
        lags[lags == ABSENT] = -1
        ths = tab[[0, 4]]
        ths[ths == ABSENT] = 0.0
        ent_lb, ent_ub = bnd[0], bnd[2]
        lagged = ((lags[1] >= 0) | (lags[4] >= 0)) & (bnd[0] != -bnd[1])
        lagged |= ((lags[2] >= 0) | (lags[5] >= 0)) & (bnd[2] != -bnd[3])
        if NNS and lagged[:NNS].any():
            e = int(np.nonzero(lagged[:NNS])[0][0])
            raise ValueError("Fixer: the bounds of node-slot entry %d differ between the scenarios of its node; "
                             "an lb / ub lag needs one bound per entry" % e)
        f64, i32, dev = torch.float64, torch.int32, ph.device

        def up(a, dt):
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
        self._tab0 = (up(ths[0], f64), up(lags[0], i32), up(lags[1], i32), up(lags[2], i32))
        self._tabk = (up(ths[1], f64), up(lags[3], i32), up(lags[4], i32), up(lags[5], i32))
        self._ent_lb, self._ent_ub = up(ent_lb, f64), up(ent_ub, f64)
        n1 = max(NNS, 1)
        self._count = torch.zeros(n1, dtype=i32, device=dev)
        self._fixed = torch.zeros(n1, dtype=i32, device=dev)
        self._fix_val = torch.zeros(n1, dtype=f64, device=dev)
        self._how_host = np.zeros(n1, dtype=np.int32)
        self._nnew = torch.zeros(1, dtype=i32, pin_memory=dev.type == "cuda")

    # verbose utility
    def _vb(self, str):
        if self.verbose and self.cylinder_rank == 0:
            print("(rank0) " + str)

    # display progress utility
    def _dp(self, str):
        if (self.dprogress or self.verbose) and self.cylinder_rank == 0:
            print("(rank0) " + str)

    # ------------------------------------------------------------ the step
    def _step(self, iter0):
        """phx_fixer_step with one rule's tables; on new fixes the flags are read
        back once and the nonants fixed (phx_fix_nonants_where).  Returns the
        number of entries fixed by this call."""
        ph = self.ph
        NNS = int(ph.NNS)
        if NNS == 0:
            return 0
        ph._settle()
        lib = ph._native
        th, nb, lbk, ubk = self._tab0 if iter0 else self._tabk
        lib.check(ph._ctx, lib.fixer_step(ph._ctx, NNS, ph._xbar_node.data_ptr(), ph._xsqbar_node.data_ptr(),
                                          th.data_ptr(), nb.data_ptr(), lbk.data_ptr(), ubk.data_ptr(),
                                          self._ent_lb.data_ptr(), self._ent_ub.data_ptr(), float(self.boundtol),
                                          int(bool(iter0)), self._count.data_ptr(), self._fixed.data_ptr(),
                                          self._fix_val.data_ptr(), self._nnew.data_ptr(), ph._stream()),
                  "fixer_step")
        if ph.device.type == "cuda":
            # (the count is in the pinned word once the stream has run the copy)
            torch.cuda.current_stream(ph.device).synchronize()
        nnew = int(self._nnew[0])
        if nnew == 0:
            return 0
        how = self._fixed.cpu().numpy()
        vals = self._fix_val.cpu().numpy()
        new = np.nonzero((how != 0) & (self._how_host == 0))[0]
        for e in new:
            self.events.append((int(ph._PHIter), int(e), int(how[e]), float(vals[e])))
        if self.verbose and self.cylinder_rank == 0:
            self._report(new, how, vals, iter0)
        self._how_host = how.copy()
        ph._fix_where_device(self._fixed, self._fix_val, host=(how, vals))
        return nnew

    def _report(self, new, how, vals, iter0):
        """The reference's "Fixed nb <scenario> <var> at <value>" lines (:177, :265)."""
        ph = self.ph
        names = ph.batch.nonant.var_names
        news = set(int(e) for e in new)
        idx = ph._xbar_idx
        for k, sname in enumerate(ph.local_scenario_names):
            for j in range(idx.shape[0]):
                e = int(idx[j, k])
                if e in news:
                    self._vb("Fixed%s %s %s %s at %s" % ("0" if iter0 else "", _HOW[int(how[e])], sname, names[j],
                                                        str(vals[e])))

    def iter0(self, local_scenarios):
        if self._no_iter0 is not None:
            print("WARNING: No Iter0 fixer tuple for s.name=", self._no_iter0)
            return
        # modelers might have already fixed variables - count those up and output the result
        fixed = getattr(self.ph, "_fixed", None)
        if fixed is not None and fixed.any() and fixed.shape[0]:
            self.fixed_prior_iter0 += int(fixed.sum()) / fixed.shape[0]
        self.fixed_so_far += float(self._step(True))
        self._dp("Unique vars fixed so far - %d (%d prior to iteration 0)"
                 % (self.fixed_so_far + self.fixed_prior_iter0, self.fixed_prior_iter0))

    def iterk(self, PHIter):
        """ Before iter k>1 solves, but after x-bar update.
        """
        if self._no_iterk is not None:
            print("MAJOR WARNING: No Iter k fixer tuple for s.name=", self._no_iterk)
            return
        self.fixed_so_far += float(self._step(False))
        self._dp("Unique vars fixed so far - %d (%d prior to iteration 0)"
                 % (self.fixed_so_far + self.fixed_prior_iter0, self.fixed_prior_iter0))

    def pre_iter0(self):
        return

    def post_iter0(self):
        """ initialize data structures; that's all we can do at this point
        """
        self.populate(self.ph.local_scenarios)

    def miditer(self):
        """ Check for fixing before in the middle of PHIter (after
        the xbar update for PHiter-1).
        """
        PHIter = self.ph._PHIter
        if PHIter == 1:  # before iter 1 solves
            self.iter0(self.ph.local_scenarios)
        else:
            self.iterk(PHIter)

    def enditer(self):
        return

    def post_everything(self):
        self._dp("Final unique vars fixed by fixer= %s" % (self.fixed_so_far))
