"""Reference path DGSQP/solvers/CA_LTV_MPC.py (``CA_LTV_MPC`` :23) -> dgsqp_amd.ltv_mpc."""
from dgsqp_amd.ltv_mpc import CA_LTV_MPC, TrackingCost, SoftStateBounds, ObstacleAvoidance  # noqa: F401
from dgsqp_amd.solver_types import CALTVMPCParams  # noqa: F401
