"""Reference path DGSQP/solvers/solver_types.py -> dgsqp_amd.solver_types (``PIDParams`` :12, ``DGSQPParams`` :92,
``DGSQPV2Params`` :130, ``CALTVMPCParams`` :203).  The parameter classes of the solvers that are out of scope (IBR, ALGAMES, PATH-MCP)
are not provided: importing them raises ImportError, as asking for those solvers should."""
from dgsqp_amd.solver_types import ControllerConfig, PIDParams, DGSQPParams, DGSQPV2Params, CALTVMPCParams  # noqa: F401
