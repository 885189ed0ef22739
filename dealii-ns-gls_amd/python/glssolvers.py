"""Nonlinear solvers and their wiring: the host-side
mirror of solver_nl.{h,cc} (NonLinearSolverLinearized / Newton / Picard) and
of the Newton lambdas of main.cc:805-864, over the device-resident operator,
GMRES and multigrid of libglsamd.so.

The nonlinear loops are control logic (a handful of scalar decisions per
iteration, as in the reference); every vector they touch stays in HBM and
every operation on them is a library call (vmult / residual / GMRES /
V-cycle) or a torch elementwise op.  The callbacks have the reference's
names and argument order, so a driver that sets them up like main.cc does
works unchanged.
"""
from __future__ import annotations

import numpy as np

import glsamd


class NonLinearSolverBase:
    """solver_nl.h: the std::function hooks the driver fills in."""

    def __init__(self):
        self.setup_jacobian = None        # (solution)
        self.setup_preconditioner = None  # (solution)
        self.evaluate_rhs = None          # (dst)
        self.evaluate_residual = None     # (dst, src)
        self.solve_with_jacobian = None   # (dst, src)
        self.postprocess = None           # (solution)
        self.history = []                 # residual l2 norms per step (the "[N] step" log)


class NonLinearSolverLinearized(NonLinearSolverBase):
    """solver_nl.cc:4-24: one linear solve around the current solution."""

    def solve(self, solution):
        import torch
        self.setup_jacobian(solution)
        rhs = torch.zeros_like(solution)
        self.evaluate_rhs(rhs)
        self.setup_preconditioner(solution)
        self.solve_with_jacobian(solution, rhs)
        return 1


class NonLinearSolverNewton(NonLinearSolverBase):
    """solver_nl.cc:26-89: Newton on the residual; the preconditioner is set
    up at the first step only when inexact_newton.  Tolerance 1e-7 and at
    most 30 steps (solver_nl.cc:29-30); exceeding them raises, as the
    reference's AssertThrow."""

    def __init__(self, inexact_newton=True, newton_tolerance=1.0e-7, newton_max_iteration=30):
        super().__init__()
        self.inexact_newton = inexact_newton
        self.newton_tolerance = newton_tolerance
        self.newton_max_iteration = newton_max_iteration

    def solve(self, solution):
        with glsamd.timer_scope("newton::solve"):  # solver_nl.cc:38
            return self._solve(solution)

    def _solve(self, solution):
        import torch
        rhs = torch.zeros_like(solution)
        inc = torch.zeros_like(solution)
        self.setup_jacobian(solution)
        self.evaluate_residual(rhs, solution)
        l2 = float(rhs.norm())
        self.history = [l2]
        it = 0
        while l2 > self.newton_tolerance:
            inc.zero_()
            if it == 0 or not self.inexact_newton:
                self.setup_preconditioner(solution)
            self.solve_with_jacobian(inc, rhs)
            solution.add_(inc)
            if self.postprocess is not None:
                self.postprocess(solution)
            self.setup_jacobian(solution)
            self.evaluate_residual(rhs, solution)
            l2 = float(rhs.norm())
            it += 1
            self.history.append(l2)
            if it > self.newton_max_iteration:
                raise RuntimeError("Newton iteration did not converge. Final residual_0 is "
                                   f"{l2}.")
        return it


class NonLinearSolverPicard(NonLinearSolverBase):
    """solver_nl.cc:91-140: fixed-point iteration on the linearized operator,
    converged when the update's l2 norm drops below 1e-7."""

    def __init__(self, picard_tolerance=1.0e-7, picard_max_iteration=30):
        super().__init__()
        self.picard_tolerance = picard_tolerance
        self.picard_max_iteration = picard_max_iteration

    def solve(self, solution):
        import torch
        rhs = torch.zeros_like(solution)
        l2, it = 1e10, 0
        self.history = []
        while l2 > self.picard_tolerance:
            tmp = solution.clone()
            self.setup_jacobian(solution)
            self.evaluate_rhs(rhs)
            self.setup_preconditioner(solution)
            self.solve_with_jacobian(solution, rhs)
            l2 = float((tmp - solution).norm())
            it += 1
            self.history.append(l2)
            if it > self.picard_max_iteration:
                raise RuntimeError("Picard iteration did not converge. Final residual_0 is "
                                   f"{l2}.")
        return it


class GMGPreconditioner:
    """PreconditionerGMG with the main.cc:815-839 setup_preconditioner step:
    interpolate_to_mg of the current solution, set_linearization_point on
    every level operator, then PreconditionerGMG::initialize (inverse
    diagonals + power-iteration relaxation factors).  Histories of the
    levels are interpolated once, at construction (main.cc:772-803)."""

    def __init__(self, meshes, cmasks, params, solution, history=None, weights=None,
                 precision="f32", **mg_kwargs):
        self.mg, self.ops = glsamd.build_gmg(meshes, cmasks, params, solution, history,
                                             weights, precision=precision, **mg_kwargs)
        self.h = self.mg.h

    def initialize(self, solution):
        import torch
        vecs = [solution.to(self.ops[-1].dtype)]
        for l in range(len(self.ops) - 1, 0, -1):
            v = self.ops[l - 1].initialize_dof_vector()
            self.mg.interpolate(l, v, vecs[0])
            vecs.insert(0, v)
        for op, v in zip(self.ops, vecs):
            op.set_linearization_point(v)
        torch.cuda.synchronize()
        self.mg.setup()

    def vmult(self, dst, src):
        return self.mg.vcycle(dst, src)


class MatrixPreconditioner:
    """PreconditionerILU / PreconditionerAMG (preconditioner.cc:5-28, 30-75;
    "preconditioner": "ILU" | "AMG", main.cc:382-395) on the assembled system
    matrix of the FP64 operator.  initialize(solution) assembles the matrix at
    the operator's current linearization point (wire_newton's setup_jacobian
    has set it, as main.cc does) and factors it: an ILU is created the first
    time and refactored on its pattern afterwards, an AMG hierarchy is rebuilt.
    LinearSolverGMRES takes the object as its preconditioner.  params: the
    keywords of glsamd.ILU / glsamd.AMG (the defaults are ILU(0), atol 1e-12,
    rtol 1; the AMG defaults with ILU smoother and coarse solver).
    device=True (ILU only): initialize never assembles on the host; the
    operator's device system matrix is factorised on the device
    (glsamd.ILU.from_operator, then refactor_from_operator)."""

    def __init__(self, op, kind="ILU", device=False, **params):
        if kind not in ("ILU", "AMG"):
            raise ValueError(f"kind: 'ILU' or 'AMG', not {kind!r}")
        if device and kind != "ILU":
            raise ValueError("device=True: the ILU only")
        self.op, self.kind, self.params, self.device = op, kind, dict(params), bool(device)
        if kind == "AMG":  # preconditioner.cc:60-61
            self.params.setdefault("smoother_type", "ILU")
            self.params.setdefault("coarse_type", "ILU")
        self.preconditioner = None

    def initialize(self, solution=None):
        with glsamd.timer_scope("gmg::initialize::" + self.kind.lower()):
            if self.device:
                if self.preconditioner is not None:
                    self.preconditioner.refactor_from_operator(self.op)
                else:
                    self.preconditioner = glsamd.ILU.from_operator(self.op, **self.params)
                return
            A = self.op.system_matrix()
            if self.kind == "ILU" and self.preconditioner is not None:
                self.preconditioner.refactor(A)
            elif self.kind == "ILU":
                self.preconditioner = glsamd.ILU(A, **self.params)
            else:
                self.preconditioner = glsamd.AMG(A, **self.params)

    def vmult(self, dst, src):
        return self.preconditioner.vmult(dst, src)


def wire_newton(solver, op, cmask, linear_solver, preconditioner=None):
    """main.cc:805-864: setup_jacobian = set_linearization_point on the fine
    operator; setup_preconditioner = GMG initialize at the solution;
    evaluate_rhs / evaluate_residual = the operator's; solve_with_jacobian =
    set_zero(src) on constrained rows, GMRES, distribute(dst) (homogeneous:
    constrained increments 0, the components node constraints eliminate take
    their rows' combination)."""
    import torch
    nc = op.dim + 1
    cm = np.asarray(cmask, dtype=np.uint8)
    con = ((cm[:, None] >> np.arange(nc)[None, :]) & 1).astype(bool).ravel()
    n_rows = op.n_node_constraints[0] if hasattr(op, "n_node_constraints") else 0
    if n_rows:
        # the eliminated rows are identity rows of the Jacobian too
        nodes = np.asarray(op.node_constraint_rows[0], dtype=np.int64)
        comps = np.asarray(op.node_constraint_rows[1], dtype=np.int64)
        con[nodes * nc + comps] = True
    con_t = torch.from_numpy(con).to("cuda")

    def setup_jacobian(src):
        op.set_linearization_point(src)

    def setup_preconditioner(solution):
        if preconditioner is not None:
            preconditioner.initialize(solution)
        linear_solver.initialize()

    def evaluate_rhs(dst):
        op.evaluate_rhs(dst)

    def evaluate_residual(dst, src):
        op.evaluate_residual(dst, src)

    def solve_with_jacobian(dst, src):
        src.masked_fill_(con_t, 0.0)
        linear_solver.solve(dst, src)
        if n_rows:
            op.distribute(dst, homogeneous=True)
        else:
            dst.masked_fill_(con_t, 0.0)

    solver.setup_jacobian = setup_jacobian
    solver.setup_preconditioner = setup_preconditioner
    solver.evaluate_rhs = evaluate_rhs
    solver.evaluate_residual = evaluate_residual
    solver.solve_with_jacobian = solve_with_jacobian
    return solver


class CylinderPostprocess:
    """SimulationCylinder::postprocess (simulation.cc:433-549): the drag and
    lift coefficients of the cylinder and the pressure difference across it,
    evaluated on the device (NavierStokesOperator.surface_force / probe, or a
    PartitionedOperator's), one line `t\\tc_D\\tc_L\\tdp\\n` appended to `path`
    per call and flushed (simulation.cc:546-548).

    op: the operator (its viscosity set), deck / mesh: the deck and the mesh
    the operator was built on.  Called by the user after a time step,
    `c_d, c_l, dp = post(t, solution)`, or assigned to
    NonLinearSolverBase.postprocess, which passes the solution only: the time
    written is then the attribute `t`, which the time loop keeps current."""

    def __init__(self, op, deck, mesh, path=None):
        self.op = op
        self.scaling = deck.force_scaling(mesh)
        cells, face_no = deck.cylinder_faces(mesh)
        op.set_force_faces(cells, face_no, 3)
        self.n_found = op.set_probe_points(deck.pressure_probe_points(mesh))
        self.dim = mesh.dim
        self.t = 0.0
        self.path = path
        self._file = open(path, "a") if path is not None else None

    def __call__(self, t, solution=None):
        if solution is None:  # NonLinearSolverBase.postprocess(solution)
            t, solution = self.t, t
        force = np.asarray(self.op.surface_force(solution), dtype=np.float64)
        values = np.asarray(self.op.probe(solution), dtype=np.float64)
        c_d, c_l = float(force[0] * self.scaling), float(force[1] * self.scaling)
        dp = float(values[0, self.dim] - values[1, self.dim])
        if self._file is not None:
            self._file.write(f"{t:g}\t{c_d:g}\t{c_l:g}\t{dp:g}\n")
            self._file.flush()
        return c_d, c_l, dp

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
