"""Specified-scenarios inner-bound spoke (cylinders/xhatspecific_bounder.py:19-100).

Its opt object is an Xhat_Eval; every new nonant vector from the hub refreshes
the nonant cache, the scenarios named in
``options["xhat_specific_options"]["xhat_scenario_dict"]`` are tried as xhat
(extensions/xhatspecific.py) and an improving objective is sent to the hub.
"""
from ..extensions.xhatspecific import XhatSpecific
from ..utils.xhat_eval import Xhat_Eval
from .spoke import InnerBoundNonantSpoke


class XhatSpecificInnerBound(InnerBoundNonantSpoke):
    converger_spoke_char = "S"

    def ib_prep(self):
        if "bundles_per_rank" in self.opt.options and self.opt.options["bundles_per_rank"] != 0:
            raise RuntimeError("xhat spokes cannot have bundles (yet)")
        if not isinstance(self.opt, Xhat_Eval):
            raise RuntimeError("XhatSpecificInnerBound must be used with Xhat_Eval.")
        xhatter = XhatSpecific(self.opt)
        xhatter.pre_iter0()
        self.opt._save_original_nonants()
        self.opt._lazy_create_solvers()
        self.opt._update_E1()
        if abs(1 - self.opt.E1) > self.opt.E1_tolerance:
            if self.opt.cylinder_rank == 0:
                print("ERROR")
                print("Total probability of scenarios was ", self.opt.E1)
                print("E1_tolerance = ", self.opt.E1_tolerance)
            quit()
        xhatter.post_iter0()
        self.opt._save_nonants()      # make the cache
        return xhatter

    def main(self):
        # what to try does not change, but the data in the scenarios should
        xhat_scenario_dict = self.opt.options["xhat_specific_options"]["xhat_scenario_dict"]
        xhatter = self.ib_prep()
        self.ib_iter = 1
        while not self.got_kill_signal():
            if self.new_nonants:
                self.opt._put_nonant_cache(self.localnonants)
                self.opt._restore_nonants_device()
                innerbound = xhatter.xhat_tryit(xhat_scenario_dict, restore_nonants=False)
                self.update_if_improving(innerbound)
            self.ib_iter += 1
