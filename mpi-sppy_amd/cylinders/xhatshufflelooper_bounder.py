"""xhatshuffle inner-bound spoke (cylinders/xhatshufflelooper_bounder.py:20-299).

Its opt object is an Xhat_Eval.  The scenarios are shuffled once (seed 42 on a
private ``random.Random``, the same on every rank); a ``ScenarioCycler`` hands
out one {non-leaf node: donor scenario} dict per loop pass, the donors'
cached nonants are tried as xhat (``XhatBase._try_one``: gathered, fixed and
solved on the device), and an improving objective goes to the hub as an inner
bound.  New nonants from the hub refresh the cache the donors are read from.

Options (``xhat_looper_options``): ``xhat_solver_options``, ``reverse``
(default True: multistage epochs alternate forward and reverse), ``iter_step``
(default 1, multistage: the ROOT branching factor).
"""
import random

from ..extensions.xhatbase import XhatBase
from ..utils.xhat_eval import Xhat_Eval
from .spoke import InnerBoundNonantSpoke


class XhatShuffleInnerBound(InnerBoundNonantSpoke):
    converger_spoke_char = "X"

    def xhatbase_prep(self):
        if "bundles_per_rank" in self.opt.options and self.opt.options["bundles_per_rank"] != 0:
            raise RuntimeError("xhat spokes cannot have bundles (yet)")
        self.verbose = self.opt.options["verbose"]
        self.solver_options = self.opt.options["xhat_looper_options"]["xhat_solver_options"]
        if not isinstance(self.opt, Xhat_Eval):
            raise RuntimeError("XhatShuffleInnerBound must be used with Xhat_Eval.")
        xhatter = XhatBase(self.opt)
        self.xhatter = xhatter
        # iter0 stuff (no iter0 solves in an xhatter)
        xhatter.pre_iter0()
        self.opt._save_original_nonants()
        self.opt._lazy_create_solvers()
        self.opt._update_E1()
        if abs(1 - self.opt.E1) > self.opt.E1_tolerance:
            raise ValueError(f"Total probability of scenarios was {self.opt.E1} "
                             f"(E1_tolerance is {self.opt.E1_tolerance})")
        xhatter.post_iter0()
        self.opt._save_nonants()      # make the cache
        self.random_seed = 42
        # a separate stream for shuffling
        self.random_stream = random.Random()

    def try_scenario_dict(self, xhat_scenario_dict):
        """One trial; True if it improved the best inner bound."""
        obj = self.xhatter._try_one(xhat_scenario_dict, solver_options=self.solver_options, verbose=False,
                                    restore_nonants=False,
                                    stage2EFsolvern=self.opt.options.get("stage2EFsolvern", None),
                                    branching_factors=self.opt.options.get("branching_factors", None))
        if self.verbose and self.opt.cylinder_rank == 0:
            print("(rank0)     %s %s%s" % ("Infeasible" if obj is None else "Feasible", xhat_scenario_dict,
                                          "" if obj is None else ", obj: %r" % obj))
        if obj is None:
            return False
        return self.update_if_improving(obj)

    def main(self):
        self.xhatbase_prep()
        looper = self.opt.options["xhat_looper_options"]
        self.reverse = looper["reverse"] if "reverse" in looper else True
        self.iter_step = looper["iter_step"] if "iter_step" in looper else None
        # all ranks the same seed, so the same order
        self.random_stream.seed(self.random_seed)
        scen_names = list(enumerate(self.opt.all_scenario_names))
        shuffled_scenarios = self.random_stream.sample(scen_names, len(scen_names))
        scenario_cycler = ScenarioCycler(shuffled_scenarios, self.opt.nonleaf_nodes, self.reverse, self.iter_step)
        xh_iter = 1
        while not self.got_kill_signal():
            # there is no iter0 here: wait for the hub's first nonants
            if self.get_serial_number() == 0:
                continue
            if self.new_nonants:
                self.opt._put_nonant_cache(self.localnonants)
                self.opt._restore_nonants_device()
            next_scendict = scenario_cycler.get_next()
            if next_scendict is not None:
                if self.try_scenario_dict(next_scendict):
                    scenario_cycler.best = next_scendict
            else:
                scenario_cycler.begin_epoch()
            xh_iter += 1


class ScenarioCycler:
    """Hands out {non-leaf node: scenario name} dicts over epochs of the
    shuffled scenarios (xhatshufflelooper_bounder.py:158-299).

    ``shuffled_scenarios``: [(index in all_scenario_names, name)] in shuffled
    order; ``nonleaves``: {name: node with kids / scenfirst / scenlast}
    (``SPBase.nonleaf_nodes``).  Two-stage: each ``get_next()`` gives the next
    scenario as the ROOT donor, stepping by ``iter_step`` (default 1), until all
    were visited; then None until ``begin_epoch()``.  Multistage: the ROOT donor
    steps by ``iter_step`` (default: the ROOT branching factor) and never
    repeats within an epoch; every other node's donor is the first scenario of
    that node at or after the ROOT donor in the cycle, replaced only once the
    cycle has passed it; with ``reverse`` (default True) epochs alternate between
    the shuffled order and its reverse.

    One difference from the reference, on purpose: its multistage ``get_next``
    returns the dict object it then updates in place for the next position
    (:268-275, :226-238), so the caller receives the NEXT position's donors and
    a dict stored as ``best`` keeps changing.  Here every call returns a dict of
    its own for the position it marks as visited: the same donors per epoch,
    starting at the epoch's first scenario instead of one step later."""

    def __init__(self, shuffled_scenarios, nonleaves, reverse, iter_step):
        root_kids = nonleaves["ROOT"].kids if "ROOT" in nonleaves else None
        if root_kids is None or len(root_kids) == 0 or root_kids[0].is_leaf:
            self._multi = False
            self._iter_shift = 1 if iter_step is None else iter_step
            self._use_reverse = False      # nothing to gain from reversing a two-stage cycle
        else:
            self._multi = True
            self.BF0 = len(root_kids)
            self._nonleaves = nonleaves
            self._iter_shift = self.BF0 if iter_step is None else iter_step
            self._use_reverse = True if reverse is None else reverse
            self._reversed = False
        self._shuffled_scenarios = shuffled_scenarios
        self._num_scenarios = len(shuffled_scenarios)
        self._begin_normal_epoch()
        self._best = None

    @property
    def best(self):
        return self._best

    @best.setter
    def best(self, value):
        self._best = value

    def _fill_nodescen_dict(self, empty_nodes):
        """Give each node of ``empty_nodes`` the first scenario of the cycle, from
        the current position on, that passes through it."""
        empty_nodes = list(empty_nodes)
        idx = self._cycle_idx
        while empty_nodes:
            if (idx == self._cycle_idx and "ROOT" in self.nodescen_dict
                    and self.nodescen_dict["ROOT"] is not None):
                # back at the start with ROOT already served: some node has no scenario
                raise RuntimeError("_fill_nodescen_dict looped over every scenario but was not able to find "
                                   "a scen for every nonleaf node.")
            sname, snum = self._shuffled_snames[idx], self._original_order[idx]
            still = []
            for ndn in empty_nodes:
                nd = self._nonleaves[ndn]
                if nd.scenfirst <= snum <= nd.scenlast:
                    self.nodescen_dict[ndn] = sname
                else:
                    still.append(ndn)
            empty_nodes = still
            idx = (idx + 1) % self._num_scenarios

    def create_nodescen_dict(self):
        """A fresh dict for the current ROOT scenario (_cur_ROOTscen up to date)."""
        if not self._multi:
            self.nodescen_dict = {"ROOT": self._cur_ROOTscen}
        else:
            self.nodescen_dict = dict()
            self._fill_nodescen_dict(self._nonleaves.keys())

    def update_nodescen_dict(self, snames_to_remove):
        """A new dict for the current ROOT scenario that keeps the donors the
        cycle has not passed yet."""
        if not self._multi:
            self.nodescen_dict = {"ROOT": self._cur_ROOTscen}
        else:
            # (a new dict: the one handed out by get_next stays as it was)
            self.nodescen_dict = dict(self.nodescen_dict)
            empty_nodes = []
            for ndn in self._nonleaves.keys():
                if self.nodescen_dict[ndn] in snames_to_remove:
                    self.nodescen_dict[ndn] = None
                    empty_nodes.append(ndn)
            self._fill_nodescen_dict(empty_nodes)

    def begin_epoch(self):
        if self._multi and self._use_reverse and not self._reversed:
            self._begin_reverse_epoch()
        else:
            self._begin_normal_epoch()

    def _begin_epoch_with(self, order):
        self._shuffled_snames = [s[1] for s in order]
        self._original_order = [s[0] for s in order]
        self._cycle_idx = 0
        self._cur_ROOTscen = self._shuffled_snames[0]
        self.create_nodescen_dict()
        self._scenarios_this_epoch = set()

    def _begin_normal_epoch(self):
        if self._multi:
            self._reversed = False
        self._begin_epoch_with(list(self._shuffled_scenarios))

    def _begin_reverse_epoch(self):
        self._reversed = True
        self._begin_epoch_with(list(reversed(self._shuffled_scenarios)))

    def get_next(self):
        """The next dict, or None when this epoch's ROOT donors are used up."""
        next_scen = self._cur_ROOTscen
        next_scendict = self.nodescen_dict
        if next_scen in self._scenarios_this_epoch:
            return None
        self._scenarios_this_epoch.add(next_scen)
        self._iter_scen()
        return next_scendict

    def _iter_scen(self):
        old_idx = self._cycle_idx
        n = self._num_scenarios
        start = (old_idx + self._iter_shift) % n
        # do not reuse a ROOT donor of this epoch: move on to the next unvisited
        # one (at most once around)
        idx = start
        while self._shuffled_snames[idx] in self._scenarios_this_epoch and (idx + 1) % n != start:
            idx = (idx + 1) % n
        self._cycle_idx = idx
        self._cur_ROOTscen = self._shuffled_snames[idx]
        if old_idx < idx:
            passed = self._shuffled_snames[old_idx:idx]
        else:
            passed = self._shuffled_snames[old_idx:] + self._shuffled_snames[:idx]
        self.update_nodescen_dict(passed)
