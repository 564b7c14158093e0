"""Host-side driver of the batched L-BFGS engine (Python flavour).

`BatchedLbfgs` mirrors `cppoptlib::solver::Lbfgs<FunctionType, m, MoreThuente>`
(reference solver/lbfgs.h:40-45 + solver/solver.h:156-231) for a *batch* of
independent problems: a public `stopping_progress`, a history size `m`, and
`minimize(objective, x0)` returning the final states and the per-problem
progress records.  PyTorch is used only for device memory and the stream; all
arithmetic runs in the HIP kernels behind the C-ABI (cppnumericalsolvers_amd/capi.py).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi


@dataclass
class Objective:
    """A device objective: id + shared parameter blob (host doubles)."""
    objective_id: int
    params: np.ndarray = field(default_factory=lambda: np.zeros(0))
    name: str = ""


def Rosenbrock(differentiability="first"):
    """Chained Rosenbrock-N (== reference src/test/verify.cc:58-69 at N = 2).  differentiability="second": the function
    declared Second mode -- Lbfgs then rebuilds its diagonal preconditioner from diag H(x) at every iterate
    (solver/lbfgs.h:116-139); on the device the diagonal comes from the functor's hess_diag (hessian_from_functor)."""
    obj = Objective(capi.OBJ_ROSENBROCK, np.zeros(0), "rosenbrock")
    if differentiability == "second":
        obj.hessian_from_functor = True
    elif differentiability != "first":
        raise ValueError("differentiability: 'first' or 'second'")
    return obj


def DiagQuadratic(a, c=0.0):
    """f(x) = sum_i a_i x_i^2 + c (README.md:21-28 quick start: a=(5,100), c=5)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    return Objective(capi.OBJ_DIAG_QUADRATIC, np.concatenate([a, [float(c)]]), "diag_quadratic")


GRAM_MAX_N, GRAM_MAX_ROWS = 256, 4096   # shapes the normal-equation kernels are built for
GRAM_AUTO_MAX_CONDITION = 3.0e2         # cond(A^T A + lam I) up to which the form is pinned to 1e-6 of the reference


def ridge_condition_bound(A, lam):
    """Upper bound of cond_2(A^T A + lam I) = lambda_max(G) / lambda_min(G), lambda_min(G) >= lam: the smaller of two
    rigorous bounds of lambda_max(G) — the largest Gershgorin row sum of |G|, and trace(G^q)^(1/q) with q = 32 / 16 / 8
    (within n^(1/q) of lambda_max; G scaled by its Gershgorin bound so the powers stay in (0, 1]) — over lam.  The same
    bound as the drop-in headers' NormalEquationConditionBound (include/cppoptlib/mi355/objectives.h)."""
    A = np.asarray(A, dtype=np.float64)
    if not lam > 0.0:
        return float("inf")
    n = A.shape[1]
    G = A.T @ A + float(lam) * np.eye(n)
    gershgorin = float(np.abs(G).sum(axis=1).max())
    if not (gershgorin > 0.0 and np.isfinite(gershgorin)):
        return float("inf")
    M, q = G / gershgorin, 1
    for _ in range(5 if n <= 64 else (4 if n <= 128 else 3)):
        M, q = M @ M, q * 2
    trace = float(np.trace(M))
    by_trace = gershgorin * trace ** (1.0 / q) * (1.0 + 1e-9) if (trace > 0.0 and np.isfinite(trace)) else gershgorin
    return min(gershgorin, by_trace) / float(lam)


def SquaredErrorRidge(A, lam, differentiability="first", matrix_cores=False, gram=False):
    """f(x) = ||A x - y_b||^2 + lam ||x||^2 (README.md:122-167 ridge example); the right-hand
    sides y_b are passed per problem (`per_problem=` of minimize / evaluate).

    differentiability="second" declares the functor Second-mode as the README prints it: Lbfgs
    then centres the two-loop recursion on the diagonal preconditioner 1/(|H_jj| + eps)
    (lbfgs.h:116-139) built from the constant Hessian diagonal
    H_jj = sum_i (2 A_ij) A_ij + lam * 2   (README `hess` of SquaredError and L2Reg)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    if isinstance(gram, str):
        if gram != "auto":
            raise ValueError("gram: True, False or 'auto'")
        # the normal-equation form inside its pinned envelope only (tests/test_relaxed_envelope.py): within 1e-6 of the
        # reference binary while cond(A^T A + lam I) <= 3e2; bounded here from above without an eigen-solve by
        # Gershgorin rows of G over lam (A^T A is positive semi-definite, so lambda_min(G) >= lam)
        gram = bool(A.shape[1] <= GRAM_MAX_N and A.shape[0] <= GRAM_MAX_ROWS and
                    ridge_condition_bound(A, lam) <= GRAM_AUTO_MAX_CONDITION)
    # matrix_cores=True: the two matrix-vector products of every evaluation run on v_mfma_f64_16x16x4_f64,
    # sixteen problems at a time (objective id 3: FMA chains instead of multiply-then-add sums; same
    # function, results within the 1e-6 tolerance; n <= 64, m <= 10)
    # gram=True: the normal-equation form (objective id 5): one Gram matrix G = A^T A + lam I for the batch, c_b = A^T y_b
    # once per problem on the matrix cores, then n^2 multiply-adds per evaluation in the ordinary Lbfgs kernel
    # (n <= 256, rows <= 4096; "auto": only inside the envelope where it is pinned to 1e-6 of the reference)
    if gram and matrix_cores:
        raise ValueError("gram=True and matrix_cores=True are two different kernels: pick one")
    oid, oname = ((capi.OBJ_SQUARED_ERROR_RIDGE_GRAM, "squared_error_ridge_gram") if gram else
                  (capi.OBJ_SQUARED_ERROR_RIDGE_MFMA, "squared_error_ridge_mfma") if matrix_cores else
                  (capi.OBJ_SQUARED_ERROR_RIDGE, "squared_error_ridge"))
    obj = Objective(oid, np.concatenate([[float(A.shape[0]), float(lam)], A.ravel()]), oname)
    if differentiability == "second":
        acc = (2.0 * A[0]) * A[0]
        for i in range(1, A.shape[0]):   # ascending rows: the order of the reference's product
            acc = acc + (2.0 * A[i]) * A[i]
        obj.hessian_diagonal = np.ascontiguousarray(acc + float(lam) * 2.0)
        # the whole (constant) Hessian 2 A^T A + 2 lam I, for the condition_hessian stopping test (progress.h:203-210)
        H = np.zeros((A.shape[1], A.shape[1]))
        for i in range(A.shape[0]):
            H = H + np.outer(2.0 * A[i], A[i])
        obj.hessian = np.ascontiguousarray(H + np.eye(A.shape[1]) * (float(lam) * 2.0))
    elif differentiability != "first":
        raise ValueError("differentiability must be 'first' or 'second'")
    return obj


def SquaredErrorRidgePerProblem(rows, lam):
    """f_b(x) = ||A_b x - y_b||^2 + lam ||x||^2 with ONE MATRIX PER PROBLEM (objective id 6): what a program computes that
    builds the README objective `SquaredError(A_b, y_b) + lam * L2Reg(n)` once per data set (README.md:126-160).  Pass
    `per_problem=ridge_per_problem_rows(As, Y)` ([B, rows * n + rows]: A_b row major, then y_b) to minimize / evaluate.
    Normal-equation form per problem (G_b, c_b on the matrix cores once, then n^2 multiply-adds per evaluation streamed from
    the problem's own G_b); fused arithmetic, First mode, More-Thuente, n <= 256, rows <= 4096."""
    return Objective(capi.OBJ_SQUARED_ERROR_RIDGE_OWN_GRAM, np.array([float(int(rows)), float(lam)]),
                     "squared_error_ridge_own_gram")


def ridge_per_problem_rows(As, Y):
    """[B, rows, n] matrices and [B, rows] right-hand sides -> the [B, rows * n + rows] per-problem rows of
    SquaredErrorRidgePerProblem."""
    As = np.asarray(As, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    B, rows, n = As.shape
    if Y.shape != (B, rows):
        raise ValueError("Y must be [B, rows]")
    return np.ascontiguousarray(np.concatenate([As.reshape(B, rows * n), Y], axis=1))


def parity_stop():
    """'parity stopping (B)' of SURVEY.md section 7: tight enough for 1e-6 parity on x*."""
    s = capi.default_stop()
    s.num_iterations = 10000
    s.x_delta = 1e-11
    s.x_delta_violations = 1
    s.f_delta = 0.0
    s.gradient_norm = 1e-8
    s.gradient_norm_relative = 1
    s.past = 0
    return s


class Context:
    """One engine context per device (owns scratch + timing events)."""

    def __init__(self, device=0, library=None):
        # `library`: path of another build of the engine, e.g. one with user objectives compiled in
        # (_build.build(output=..., user_objectives=[...])); default: the in-tree library
        self._lib = capi.load(library)   # (imports torch before mapping the engine: one HIP runtime per process)
        h = C.c_void_p()
        capi.check(self._lib.mi355_lbfgs_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi355_lbfgs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


class Trace:
    """Opt-in per-iteration trace of chosen problems (mi355_lbfgs_trace): what `Solver::step_callback_` of the
    reference observes (solver/solver.h:197, :222), recorded on the device.  `problems`: batch indices (at most 64);
    `capacity`: iterations kept per problem (a ring: the last `capacity` are kept); with_x / with_g: also keep the
    iterate / its gradient after every traced iteration.  Pass it to `minimize(..., trace=t)`; after synchronising,
    `t.history(i)` returns the records of traced problem i in chronological order (+ x, g arrays)."""

    def __init__(self, problems, capacity, n, device, with_x=True, with_g=False):
        import torch
        self.problems = np.ascontiguousarray(problems, dtype=np.int64)
        if not (1 <= self.problems.size <= capi.MAX_TRACED):
            raise ValueError("1..%d traced problems" % capi.MAX_TRACED)
        self.capacity, self.n = int(capacity), int(n)
        K = self.problems.size
        self.records = torch.zeros(K * self.capacity * capi.TRACE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self.x = torch.zeros(K, self.capacity, n, dtype=torch.float64, device=device) if with_x else None
        self.g = torch.zeros(K, self.capacity, n, dtype=torch.float64, device=device) if with_g else None
        self.written = torch.zeros(K, dtype=torch.int32, device=device)
        self._c = capi.Trace()
        self._c.count, self._c.capacity = K, self.capacity
        self._c.problems = self.problems.ctypes.data_as(C.POINTER(C.c_int64))
        self._c.records = self.records.data_ptr()
        self._c.x = self.x.data_ptr() if with_x else None
        self._c.g = self.g.data_ptr() if with_g else None
        self._c.written = self.written.data_ptr()

    def c_pointer(self):
        return C.addressof(self._c)

    def history(self, i):
        """(records, x, g) of traced problem i, oldest kept iteration first."""
        w = int(self.written[i].item())
        rec = self.records.cpu().numpy().view(capi.TRACE_RECORD_DTYPE).reshape(-1, self.capacity)[i]
        kept = min(w, self.capacity)
        idx = [(t - 1) % self.capacity for t in range(w - kept + 1, w + 1)]
        x = self.x[i].cpu().numpy()[idx] if self.x is not None else None
        g = self.g[i].cpu().numpy()[idx] if self.g is not None else None
        return rec[idx], x, g


def _float64_only(solver, dtype):
    """The solvers other than BatchedLbfgs compute in float64 only."""
    if dtype is not None and str(dtype) != "torch.float64":
        raise ValueError("%s computes in float64 only: dtype=torch.float32 is built for BatchedLbfgs (its native float "
                         "path); got dtype=%s" % (type(solver).__name__, dtype))


class BatchedLbfgs:
    """Batched `Lbfgs<F, m>` — one problem per wavefront segment on the GPU.

    stopping_progress: capi.Stop (defaults to DefaultStoppingSolverProgress).
    m: history size (reference default 10).
    lanes_per_problem / elems_per_lane: optional explicit wavefront mapping.
    dtype: torch.float64 (default: every computation in fp64) or torch.float32 — the native float path
        (mi355_lbfgs_minimize_batch_f32): `minimize` / `evaluate` take and return float32 CUDA tensors, `minimize_host`
        float32 numpy arrays; More-Thuente, exact arithmetic, Rosenbrock / DiagQuadratic, n <= 256.  What that path does
        not build is refused by the library with its reason (EngineError).  Only this class takes float32;
        `minimize_callable` / `LbfgsAskTell` on it run the float ask/tell path (mi355_lbfgs_ask_tell_f32_*) on any
        float32 objective the caller evaluates.
    """

    _entry = "mi355_lbfgs_minimize_batch"  # C-ABI entry point (subclasses: other solvers of the same shape)

    def __init__(self, m=10, stopping_progress=None, device=0, lanes_per_problem=0, elems_per_lane=0,
                 context=None, history_placement=0, linesearch="more_thuente", arithmetic="default",
                 condition_hessian=0.0, dtype=None):
        import torch
        self._torch = torch
        self.dtype = torch.float64 if dtype is None else dtype
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype must be torch.float64 or torch.float32")
        if self.dtype == torch.float32 and type(self) is not BatchedLbfgs:
            raise ValueError("%s computes in float64 only: dtype=torch.float32 is built for BatchedLbfgs"
                             % type(self).__name__)
        self._f32 = self.dtype == torch.float32
        self._np_dtype = np.float32 if self._f32 else np.float64
        self.m = int(m)
        self.stopping_progress = stopping_progress or capi.default_stop()
        self.lanes_per_problem = int(lanes_per_problem)
        self.elems_per_lane = int(elems_per_lane)
        self.history_placement = int(history_placement)
        # the LineSearch template argument of the reference's Lbfgs (lbfgs.h:41)
        self.linesearch = {"more_thuente": capi.LS_MORE_THUENTE, "hager_zhang": capi.LS_HAGER_ZHANG}[linesearch]
        # mi355_arithmetic: "exact" (no FMA, bit-identical to the oracle's butterfly policy), "fma" (fused
        # multiply-adds in the inner products, axpys, trial point and objective; bit-identical to the oracle's
        # butterfly_fma policy, within 1e-6 of the reference-order solve), "default" = fma where it is built
        self.arithmetic = {"default": capi.ARITH_DEFAULT, "exact": capi.ARITH_EXACT, "fma": capi.ARITH_FMA}[arithmetic]
        # stopping_progress.condition_hessian of the reference (progress.h:110): Second-mode objectives only, 0 = off
        self.condition_hessian = float(condition_hessian)
        self.ctx = context or Context(device)
        self.device = torch.device("cuda", self.ctx.device)

    # -- helpers -----------------------------------------------------------
    def _desc(self, objective, n, per_problem=None, per_problem_stride=0):
        d = capi.Desc()
        d.objective = objective.objective_id
        d.linesearch = self.linesearch
        d.n = int(n)
        d.m = self.m
        p = np.ascontiguousarray(objective.params, dtype=np.float64)
        self._params_keepalive = p
        d.objective_params = p.ctypes.data_as(C.POINTER(C.c_double)) if p.size else None
        d.n_params = int(p.size)
        d.per_problem_data = per_problem
        d.per_problem_stride = int(per_problem_stride)
        d.lanes_per_problem = self.lanes_per_problem
        d.elems_per_lane = self.elems_per_lane
        d.history_placement = self.history_placement
        d.arithmetic = self.arithmetic
        if getattr(objective, "hessian_from_functor", False):
            d.hessian_from_functor = 1
            d.hessian_condition_stop = self.condition_hessian   # (n <= 64: the kernel evaluates cond H(x) of every iterate)
        h = getattr(objective, "hessian_diagonal", None)
        if h is not None:
            if h.shape != (int(n),):
                raise ValueError("hessian_diagonal must hold n entries")
            self._hess_keepalive = h
            d.hessian_diagonal = h.ctypes.data_as(C.POINTER(C.c_double))
            H = getattr(objective, "hessian", None)
            if H is not None:
                cond = C.c_double()
                capi.check(self.ctx._lib.mi355_lbfgs_hessian_condition(H.ctypes.data, int(n), C.byref(cond)))
                d.hessian_condition = cond.value
                self.last_hessian_condition = cond.value
            d.hessian_condition_stop = self.condition_hessian
        d.stop = self.stopping_progress
        return d

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _config_args(self):
        """What the solver's entry points take between the desc and B: nothing here, a config struct in _ConfiguredSolver."""
        return ()

    # -- API ---------------------------------------------------------------
    def _on_device(self, t, what):
        """The C entry points dereference raw pointers on the context's device."""
        if t.device != self.device:
            raise ValueError("%s lives on %s, the solver's context on %s" % (what, t.device, self.device))

    def _pp_device(self, per_problem, B):
        if per_problem is None:
            return None, 0
        torch = self._torch
        if per_problem.dtype != torch.float64 or per_problem.dim() != 2 or per_problem.shape[0] != B \
                or not per_problem.is_cuda:
            raise ValueError("per_problem must be a [B, stride] float64 CUDA tensor")
        self._on_device(per_problem, "per_problem")
        pp = per_problem.contiguous()
        self._pp_keepalive = pp
        return pp.data_ptr(), pp.shape[1]

    def minimize(self, objective, x0, want_gradient=True, want_progress=True, per_problem=None, trace=None):
        """Batched Solver::Minimize.  x0: [B, n] float64 tensor on this device.

        Returns (x, f, g, progress) — device tensors; progress is a uint8 tensor
        of B*40 bytes viewable with `progress_to_numpy`.  Asynchronous on the
        current stream.
        """
        torch = self._torch
        if x0.dtype != self.dtype or x0.dim() != 2 or not x0.is_cuda:
            raise ValueError("x0 must be a [B, n] %s CUDA tensor" % ("float32" if self._f32 else "float64"))
        self._on_device(x0, "x0")
        x0 = x0.contiguous()
        B, n = x0.shape
        x = torch.empty_like(x0)
        f = torch.empty(B, dtype=self.dtype, device=x0.device)
        g = torch.empty_like(x0) if want_gradient else None
        prog = torch.empty(B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=x0.device) \
            if want_progress else None
        d = self._desc(objective, n, *self._pp_device(per_problem, B))
        if trace is not None:
            self._trace_keepalive = trace
            d.trace = trace.c_pointer()
        capi.check(getattr(self.ctx._lib, self._entry + ("_f32" if self._f32 else ""))(
            self.ctx.handle, C.byref(d), *self._config_args(), B, x0.data_ptr(), x.data_ptr(), f.data_ptr(),
            g.data_ptr() if g is not None else None, prog.data_ptr() if prog is not None else None,
            self._stream()))
        return x, f, g, prog

    def minimize_host(self, objective, x0, per_problem=None):
        """Same through the host-pointer entry point (numpy in, numpy out, synchronous)."""
        if self._f32 and np.asarray(x0).dtype != np.float32:
            raise ValueError("x0 must be a [B, n] float32 array")
        x0 = np.ascontiguousarray(x0, dtype=self._np_dtype)
        B, n = x0.shape
        pp_ptr, pp_stride = None, 0
        if per_problem is not None:
            pp = np.ascontiguousarray(per_problem, dtype=np.float64)
            self._pp_keepalive = pp
            pp_ptr, pp_stride = pp.ctypes.data, pp.shape[1]
        x = np.empty_like(x0)
        g = np.empty_like(x0)
        f = np.empty(B, dtype=self._np_dtype)
        prog = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
        d = self._desc(objective, n, pp_ptr, pp_stride)
        capi.check(getattr(self.ctx._lib, self._entry + ("_f32_host" if self._f32 else "_host"))(
            self.ctx.handle, C.byref(d), *self._config_args(), B, x0.ctypes.data, x.ctypes.data, f.ctypes.data,
            g.ctypes.data, prog.ctypes.data))
        return x, f, g, prog

    def evaluate(self, objective, x, per_problem=None):
        """One objective evaluation per row of x (device functor parity tests)."""
        torch = self._torch
        self._on_device(x, "x")
        if self._f32 and x.dtype != torch.float32:
            raise ValueError("x must be a [B, n] float32 CUDA tensor")
        x = x.contiguous()
        B, n = x.shape
        f = torch.empty(B, dtype=self.dtype, device=x.device)
        g = torch.empty_like(x)
        d = self._desc(objective, n, *self._pp_device(per_problem, B))
        entry = self.ctx._lib.mi355_lbfgs_eval_batch_f32 if self._f32 else self.ctx._lib.mi355_lbfgs_eval_batch
        capi.check(entry(
            self.ctx.handle, C.byref(d), B, x.data_ptr(), f.data_ptr(), g.data_ptr(), self._stream()))
        return f, g

    def hz_search(self, objective, x, direction, alpha_init, per_problem=None):
        """One HagerZhang::Search (hager_zhang.h:100-116) per row of x along the rows of `direction`;
        returns the accepted x, f, g, the step widths and the evaluation counts."""
        torch = self._torch
        for t, what in ((x, "x"), (direction, "direction"), (alpha_init, "alpha_init")):
            self._on_device(t, what)
        x = x.contiguous()
        direction = direction.contiguous()
        B, n = x.shape
        a0 = alpha_init.contiguous()
        xo, go = torch.empty_like(x), torch.empty_like(x)
        fo = torch.empty(B, dtype=torch.float64, device=x.device)
        ao = torch.empty(B, dtype=torch.float64, device=x.device)
        nf = torch.empty(B, dtype=torch.int32, device=x.device)
        d = self._desc(objective, n, *self._pp_device(per_problem, B))
        capi.check(self.ctx._lib.mi355_lbfgs_hz_search_batch(
            self.ctx.handle, C.byref(d), B, x.data_ptr(), direction.data_ptr(), a0.data_ptr(), xo.data_ptr(),
            fo.data_ptr(), go.data_ptr(), ao.data_ptr(), nf.data_ptr(), self._stream()))
        return xo, fo, go, ao, nf

    def fill_x0(self, B, n, kind="std", seed=20260923, first_problem=0):
        """Seeded synthetic start points generated on the device."""
        torch = self._torch
        x0 = torch.empty(B, n, dtype=torch.float64, device=self.device)
        capi.check(self.ctx._lib.mi355_lbfgs_fill_x0(
            self.ctx.handle, 0 if kind == "std" else 1, seed, first_problem, B, n, x0.data_ptr(),
            self._stream()))
        return x0

    def minimize_callable(self, fn, x0, check_every=1, max_rounds=None, compact_every=None):
        """Batched Solver::Minimize of an objective the CALLER evaluates (ask/tell, `LbfgsAskTell`): `fn(X)` takes the
        [B, n] CUDA tensor of the points to evaluate (of the solver's dtype: float64, or float32 on the native float
        path of BatchedLbfgs) and returns (f [B], g [B, n]) of that dtype — or f alone, and the gradient
        is then torch.autograd.grad(f.sum(), X) on a leaf that requires grad (the problems are independent, so the
        sum's gradient is the per-problem gradient; in float32 autograd differentiates in float32).  X is the solver's own buffer: read it, do not keep or write it.
        check_every=k reads the active count back every k rounds (a round on a finished batch changes nothing);
        max_rounds: RuntimeError when the batch is still active after that many rounds.
        compact_every=k (None: off, and everything above is the whole story): the loop keeps the LIST of the problems
        that have not finished (`LbfgsAskTell.compact`), rebuilt every k rounds, and calls `fn(X, ids)` with X [listed, n]
        — the points of the listed problems only — and ids [listed] int64, their numbers, ascending: an objective with
        per-problem data indexes it by ids, and a finished problem costs no evaluation after the next compaction.  f is
        [listed], g [listed, n] (or f alone, as above).  The loop ends when a compaction lists nothing; check_every is
        ignored then: the active count is read every round, so fn runs exactly as many rounds as with check_every=1.
        The results are those of the loop without a list, bit for bit.
        A compaction is three small kernels, a read-back and a copy of the kept rows (about 37 us): k = 1 drops a
        finished problem at once, a larger k spreads that cost over k rounds.  Measured on 65 536 x Rosenbrock-32
        (profiles/ask_tell_compact_rounds.txt): fn sees 15.7 % of batch x rounds at k = 1 and 16.1 % at k = 16; with
        the cheapest fn there is (one small kernel) no k beats the loop without a list at check_every=16, and k = 16 or
        64 beats check_every=1 by 4 - 6 %.  Use k = 16 when fn's cost grows with its rows; leave it None when fn is cheap.
        Returns (x, f, g, progress) like `minimize`."""
        if int(check_every) < 1:
            raise ValueError("check_every must be >= 1")
        if compact_every is not None and int(compact_every) < 1:
            raise ValueError("compact_every must be >= 1 (None: no list)")
        torch = self._torch
        value_only = [None]   # which of the two forms fn has: the first round tells

        def evaluate(X, *ids):
            if value_only[0] is None:
                with torch.no_grad():
                    out = fn(X, *ids)
                value_only[0] = not isinstance(out, (tuple, list))
                if not value_only[0]:
                    return out
            if not value_only[0]:
                return fn(X, *ids)
            leaf = X.detach().requires_grad_(True)
            f = fn(leaf, *ids)
            (g,) = torch.autograd.grad(f.sum(), leaf)
            return f.detach(), g

        if compact_every is not None:
            with self._ask_tell(x0) as at:
                rounds = 0
                while at.compact() > 0:
                    for _ in range(int(compact_every)):
                        f, g = evaluate(at.x, at.ids)
                        rounds += 1
                        active = at.tell(f, g)   # (read every round: fn is never called on a finished batch)
                        if active == 0:
                            break
                        if max_rounds is not None and rounds >= int(max_rounds):
                            raise RuntimeError("minimize_callable: %d problems still active after max_rounds = %d rounds"
                                               % (active, int(max_rounds)))
                return at.results()

        with self._ask_tell(x0) as at:
            rounds = 0
            while at.B > 0:
                f, g = evaluate(at.x)
                rounds += 1
                if rounds % int(check_every) == 0:
                    if at.tell(f, g) == 0:
                        break
                else:
                    at.tell(f, g, wait=False)
                if max_rounds is not None and rounds >= int(max_rounds):
                    if at.active == 0:
                        break
                    raise RuntimeError("minimize_callable: %d problems still active after max_rounds = %d rounds"
                                       % (at.active, int(max_rounds)))
            return at.results()

    def _ask_tell(self, x0):
        """The ask/tell handle of this solver class (minimize_callable's)."""
        return LbfgsAskTell(self, x0)

    def last_kernel_ms(self):
        ms = C.c_float()
        capi.check(self.ctx._lib.mi355_lbfgs_last_kernel_ms(self.ctx.handle, C.byref(ms)))
        return float(ms.value)

    def last_arithmetic(self):
        """'exact' or 'fma': what the most recent solve on this solver's context ran with."""
        v = C.c_int32()
        capi.check(self.ctx._lib.mi355_lbfgs_last_arithmetic(self.ctx.handle, C.byref(v)))
        return {capi.ARITH_EXACT: "exact", capi.ARITH_FMA: "fma"}[v.value]

    def last_launch(self):
        v = [C.c_int32() for _ in range(6)]
        capi.check(self.ctx._lib.mi355_lbfgs_last_launch(self.ctx.handle, *[C.byref(t) for t in v]))
        out = dict(zip(("lanes_per_problem", "elems_per_lane", "blocks", "threads", "lds_bytes",
                        "y_columns_in_registers"),
                       [t.value for t in v]))
        # "lean": the solve kernel with the call's options fixed at compile time (csrc/dispatch_lean.hip); same bits
        k = C.c_int32()
        capi.check(self.ctx._lib.mi355_lbfgs_last_kernel_variant(self.ctx.handle, C.byref(k)))
        out["kernel"] = {0: "general", 1: "lean"}[k.value]
        return out


class _DeviceArray:
    """A device buffer the library owns, described through __cuda_array_interface__ so that torch.as_tensor makes a
    tensor VIEW of it (no copy); `owner` keeps the allocation alive for as long as the view exists."""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2,
                                             strides=None)


class LbfgsAskTell:
    """One ask/tell solve (mi355_lbfgs_ask_tell_*): `Lbfgs<F, m, MoreThuente>::Minimize` of B problems whose objective
    the caller evaluates.  The solver state of all problems lives on the device; every `tell` runs one kernel that takes
    each problem to its next evaluation.

        at = amd.LbfgsAskTell(solver, x0)          # solver: a BatchedLbfgs (m, stopping_progress, mapping, dtype)
        while at.tell(*my_value_and_gradient(at.x)) > 0:
            pass
        x, f, g, progress = at.results()

    .x: the [B, n] float64 tensor VIEW of the evaluation buffer (no copy; valid until close()); rows of finished
    problems hold their returned x, and what is handed back for them is never read.  A solver built with
    dtype=torch.float32 runs the native float path (mi355_lbfgs_ask_tell_f32_*): x0, .x, f, g and the results are
    float32 then, and a tensor of the other dtype is a ValueError in both directions.  Above n = 256 a float64 solver
    runs the workgroup-per-problem handle (mi355_lbfgs_ask_tell_wide_*: same protocol, same results as `minimize` at that
    n bit for bit when fn is `solver.evaluate`; B ((3 + 2 m) n + n) 8 bytes of device memory; the library's mapping only);
    a float32 solver is refused there.  A solver configured with what the
    path does not build (Hager-Zhang, arithmetic="fma", y history in registers, condition_hessian) raises the
    library's message (EngineError).  Everything runs on the current stream of the solver's device."""

    _prefix = "mi355_lbfgs_ask_tell_"

    _prefix_f32 = "mi355_lbfgs_ask_tell_f32_"   # the handle type of a float32 solver
    _listed_suffix = "lbfgs"                    # mi355_ask_tell_compact_lbfgs[_f32], mi355_ask_tell_ids_lbfgs[_f32]

    _prefix_wide = "mi355_lbfgs_ask_tell_wide_"   # ... of a float64 BatchedLbfgs above n = 256 (a workgroup per problem)
    _wide = False

    def _call(self, name, *args):
        prefix = self._prefix_f32 if self._f32 else (self._prefix_wide if self._wide else self._prefix)
        capi.check(getattr(self._lib, prefix + name)(*args))

    def _check_solver(self, solver):
        if type(solver) is not BatchedLbfgs:
            raise TypeError("LbfgsAskTell takes a BatchedLbfgs (BatchedLbfgsb has LbfgsbAskTell; the other solvers have "
                            "no ask/tell form)")

    def _create(self, solver, d, x0, h):
        self._call("create", solver.ctx.handle, C.byref(d), self.B, x0.data_ptr(), solver._stream(), C.byref(h))

    def __init__(self, solver, x0):
        self._h = None
        self._check_solver(solver)
        torch = solver._torch
        self._f32 = bool(solver._f32)
        self._dtype = solver.dtype
        self._dtype_name = "float32" if self._f32 else "float64"
        if x0.dtype != self._dtype or x0.dim() != 2 or not x0.is_cuda:
            raise ValueError("x0 must be a [B, n] %s CUDA tensor: the solver computes in %s"
                             % (self._dtype_name, self._dtype_name))
        solver._on_device(x0, "x0")
        x0 = x0.contiguous()
        self.solver = solver
        self.B, self.n = (int(v) for v in x0.shape)
        # above n = 256 a float64 BatchedLbfgs runs the workgroup-per-problem handle; float32 keeps its refusal
        self._wide = type(solver) is BatchedLbfgs and not self._f32 and self.n > capi.MAX_N
        self._lib = solver.ctx._lib
        d = solver._desc(Objective(capi.OBJ_ROSENBROCK, np.zeros(0), "caller"), self.n)
        d.hessian_condition_stop = solver.condition_hessian
        h = C.c_void_p()
        self._create(solver, d, x0, h)
        self._h = h
        p = C.c_void_p()
        self._call("x", self._h, C.byref(p))
        self._x_ptr = p.value
        self.ids = None          # compact(): the [listed] int64 view of the list
        self._listed = self.B    # rows of .x / f / g: B, or the length of the list
        self.x = self._x_view(self.B)
        self._call("active", self._h, C.byref(p))
        self._active_dev = torch.as_tensor(_DeviceArray(p.value, (1,), "<i8", self), device=solver.device)

    def _rows(self, t, shape, what):
        torch = self.solver._torch
        if not isinstance(t, torch.Tensor) or t.dtype != self._dtype or tuple(t.shape) != shape or not t.is_cuda:
            raise ValueError("%s must be a %s %s CUDA tensor" % (what, list(shape), self._dtype_name))
        self.solver._on_device(t, what)
        return t.detach().contiguous()

    def _x_view(self, rows):
        """the first `rows` rows of the evaluation buffer as a tensor VIEW"""
        torch = self.solver._torch
        if rows == 0:
            return torch.empty(0, self.n, dtype=self._dtype, device=self.solver.device)
        return torch.as_tensor(_DeviceArray(self._x_ptr, (rows, self.n), "<f4" if self._f32 else "<f8", self),
                               device=self.solver.device)

    def _call_listed(self, name, *args):
        """mi355_ask_tell_<name>_<handle type>: the calls of the listed mode"""
        if self._wide:   # (named after its handle type: mi355_lbfgs_ask_tell_wide_compact / _ids)
            return self._call(name, *args)
        suffix = self._listed_suffix + ("_f32" if self._f32 else "")
        capi.check(getattr(self._lib, "mi355_ask_tell_%s_%s" % (name, suffix))(*args))

    def compact(self):
        """Rebuilds the list of the problems that have not finished (mi355_ask_tell_compact_*; waits for the stream) and
        returns its length `listed`.  Afterwards .ids is the [listed] int64 view of the problems' numbers, ascending, .x
        the [listed, n] view of the SAME buffer — row s is the point to evaluate for problem ids[s] — and tell() takes
        f [listed], g [listed, n].  A problem that finishes later stays listed until the next compact().  results() is
        always all B problems, in problem order, and equals the uncompacted solve's bit for bit."""
        if self._h is None:
            raise RuntimeError("this %s is closed" % type(self).__name__)
        torch = self.solver._torch
        count = C.c_int64(-1)
        self._call_listed("compact", self._h, C.byref(count), self.solver._stream())
        p, listed = C.c_void_p(), C.c_int64(-1)
        self._call_listed("ids", self._h, C.byref(p), C.byref(listed))
        self._listed = int(listed.value)
        assert self._listed == int(count.value)
        self.x = self._x_view(self._listed)
        self.ids = torch.as_tensor(_DeviceArray(p.value, (self._listed,), "<i8", self), device=self.solver.device) \
            if self._listed > 0 else torch.empty(0, dtype=torch.int64, device=self.solver.device)
        return self._listed

    def tell(self, f, g, wait=True):
        """Hands the values f [B] and gradients g [B, n] at the rows of .x to the solver and advances every problem to
        its next evaluation (after compact(): f [listed], g [listed, n], and only the listed problems run).
        wait=True: returns the number of problems still active (waits for the stream);
        wait=False: returns None and nothing waits (`.active` reads the count later)."""
        if self._h is None:
            raise RuntimeError("this %s is closed" % type(self).__name__)
        f = self._rows(f, (self._listed,), "f")
        g = self._rows(g, (self._listed, self.n), "g")
        count = C.c_int64(-1)
        self._call("step", self._h, f.data_ptr(), g.data_ptr(), C.byref(count) if wait else None, self.solver._stream())
        return int(count.value) if wait else None

    @property
    def active(self):
        """The number of problems that have not finished (reads the device counter: waits for the stream)."""
        if self._h is None:
            raise RuntimeError("this %s is closed" % type(self).__name__)
        return int(self._active_dev.item())

    def results(self):
        """(x, f, g, progress) like BatchedLbfgs.minimize: the current iterate of every problem (the returned state of
        a finished one); at any time between two tells."""
        if self._h is None:
            raise RuntimeError("this %s is closed" % type(self).__name__)
        torch = self.solver._torch
        dev = self.solver.device
        x = torch.empty(self.B, self.n, dtype=self._dtype, device=dev)
        g = torch.empty(self.B, self.n, dtype=self._dtype, device=dev)
        f = torch.empty(self.B, dtype=self._dtype, device=dev)
        prog = torch.empty(self.B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._call("results", self._h, x.data_ptr(), f.data_ptr(), g.data_ptr(), prog.data_ptr(), self.solver._stream())
        return x, f, g, prog

    def close(self):
        """Frees the device state (waits for the device); .x must not be used afterwards."""
        if getattr(self, "_h", None) is not None:
            h, self._h = self._h, None
            self.x = self.ids = self._active_dev = None
            self._call("destroy", h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedBfgs(BatchedLbfgs):
    """Batched dense `Bfgs<F, LineSearch>` (reference solver/bfgs.h): the same driver, line searches and
    stopping tests with an explicit inverse-Hessian approximation per problem; n <= 64."""
    _entry = "mi355_bfgs_minimize_batch"

    def __init__(self, stopping_progress=None, device=0, context=None, linesearch="more_thuente",
                 lanes_per_problem=0, elems_per_lane=0, dtype=None):
        _float64_only(self, dtype)
        # mapping 0 x 0: the library's choice (one column of H per lane at the padded widths 32 and 64); an explicit split
        # must cover exactly the padded width with a built shape (include/mi355_lbfgs.h) — same bits either way
        super().__init__(m=1, stopping_progress=stopping_progress, device=device, context=context,
                         linesearch=linesearch, arithmetic="exact", lanes_per_problem=lanes_per_problem,
                         elems_per_lane=elems_per_lane)


class _ConfiguredSolver(BatchedLbfgs):
    """What TrustRegionNewton, NewtonDescent, NelderMead and the two first-order solvers share on top of BatchedLbfgs: their
    entry points (`_entry`, `_entry` + "_host") take the solver's config struct after the desc — `self.config`, or nothing
    where the solver has none (GradientDescent) — and their host entry points take no per-problem data."""

    def _config_args(self):
        config = getattr(self, "config", None)
        return () if config is None else (C.byref(config),)

    def minimize_host(self, objective, x0, per_problem=None):
        """Same through the host-pointer entry point (numpy in, numpy out, synchronous)."""
        if per_problem is not None:
            raise ValueError("per-problem data: use minimize() with device tensors")
        return super().minimize_host(objective, x0)


class BatchedTrustRegionNewton(_ConfiguredSolver):
    """Batched `TrustRegionNewton<F>` (reference solver/trust_region_newton.h): one Hessian per outer step, CG-Steihaug
    on the quadratic model, the agreement ratio, the radius update and the in-step rejection loop; n <= 64, objectives
    whose device functor has a hess_full (Rosenbrock, DiagQuadratic, user functors built with trust_region=True).

    The keyword arguments are the fields of TrustRegionNewtonConfig (same names and defaults); `condition_hessian` is
    stopping_progress.condition_hessian (0 = off).  progress.sum_k holds the solve's total CG iterations."""
    _entry = "mi355_trust_region_newton_minimize_batch"

    def __init__(self, stopping_progress=None, device=0, context=None, lanes_per_problem=0, condition_hessian=0.0,
                 dtype=None, **config):
        _float64_only(self, dtype)
        super().__init__(m=1, stopping_progress=stopping_progress, device=device, context=context,
                         arithmetic="exact", lanes_per_problem=lanes_per_problem, condition_hessian=condition_hessian)
        self.config = capi.default_trust_region_config(**config)

    def _desc(self, objective, n, per_problem=None, per_problem_stride=0):
        d = super()._desc(objective, n, per_problem, per_problem_stride)
        d.hessian_from_functor = 0     # (H(x) always comes from the device functor's hess_full)
        d.hessian_diagonal = None
        d.hessian_condition = 0.0
        d.hessian_condition_stop = self.condition_hessian
        return d


class BatchedNewtonDescent(BatchedTrustRegionNewton):
    """Batched `NewtonDescent<F>` (reference solver/newton_descent.h): per step d = (H + safe_guard I).lu().solve(-g) and
    the Armijo search with the Newton curvature term (linesearch/armijo.h, Armijo<F, 2>) from alpha = 1; n <= 64,
    objectives whose device functor has a hess_full (Rosenbrock, DiagQuadratic, user functors built with
    newton_descent=True).

    safe_guard, armijo_c, armijo_rho are the reference's constants (defaults 1e-5, 0.2, 0.9); `condition_hessian` is
    stopping_progress.condition_hessian (0 = off).  progress.sum_k holds the solve's total trial points.  The search is
    bounded where the reference's is not: it also ends when alpha * armijo_rho == alpha (include/mi355_lbfgs.h)."""
    _entry = "mi355_newton_descent_minimize_batch"

    def __init__(self, stopping_progress=None, device=0, context=None, lanes_per_problem=0, condition_hessian=0.0,
                 dtype=None, **config):
        _float64_only(self, dtype)
        BatchedLbfgs.__init__(self, m=1, stopping_progress=stopping_progress, device=device, context=context,
                              arithmetic="exact", lanes_per_problem=lanes_per_problem,
                              condition_hessian=condition_hessian)
        self.config = capi.default_newton_descent_config(**config)


class BatchedGradientDescent(_ConfiguredSolver):
    """Batched `GradientDescent<F>` (reference solver/gradient_descent.h with the More-Thuente search): per step the search
    runs along -g from alpha = 1 and the step is x - rate g; n <= 256, x and g in registers; Rosenbrock, DiagQuadratic
    and user functors built with first_order=True.  progress.sum_k holds the solve's total trial points."""
    _entry = "mi355_gradient_descent_minimize_batch"
    _config = None

    def __init__(self, stopping_progress=None, device=0, context=None, lanes_per_problem=0, elems_per_lane=0,
                 dtype=None):
        _float64_only(self, dtype)
        super().__init__(m=1, stopping_progress=stopping_progress, device=device, context=context, arithmetic="exact",
                         lanes_per_problem=lanes_per_problem, elems_per_lane=elems_per_lane)

    def _desc(self, objective, n, per_problem=None, per_problem_stride=0):
        d = super()._desc(objective, n, per_problem, per_problem_stride)
        d.hessian_from_functor = 0     # (first-order solvers: no Hessian field is read)
        d.hessian_diagonal = None
        d.hessian_condition = 0.0
        d.hessian_condition_stop = 0.0
        return d


class BatchedConjugatedGradientDescent(BatchedGradientDescent):
    """Batched `ConjugatedGradientDescent<F>` (reference solver/conjugated_gradient_descent.h): d = -g at the first step,
    then the Fletcher-Reeves beta = (g.g) / (g_prev.g_prev) and d = -g + beta d, with the backtracking search
    Armijo<F, 1> (linesearch/armijo.h) from alpha = 1; the same objectives and sizes as BatchedGradientDescent.

    armijo_c, armijo_rho, armijo_alpha_min are the reference's constants (defaults 0.2, 0.9, 1e-8)."""
    _entry = "mi355_conjugated_gradient_descent_minimize_batch"

    def __init__(self, stopping_progress=None, device=0, context=None, lanes_per_problem=0, elems_per_lane=0,
                 armijo_c=None, armijo_rho=None, armijo_alpha_min=None, dtype=None):
        _float64_only(self, dtype)
        super().__init__(stopping_progress=stopping_progress, device=device, context=context,
                         lanes_per_problem=lanes_per_problem, elems_per_lane=elems_per_lane)
        given = dict(c=armijo_c, rho=armijo_rho, alpha_min=armijo_alpha_min)
        self._config = capi.default_armijo_config(**{k: float(v) for k, v in given.items() if v is not None})

    @property
    def config(self):
        return self._config


class BatchedNelderMead(_ConfiguredSolver):
    """Batched `NelderMead<F>` (reference solver/nelder_mead.h): the derivative-free simplex method, one problem per
    wavefront segment with the simplex and its vertex values in LDS; n <= 64, Rosenbrock, DiagQuadratic and user functors
    built with nelder_mead=True.

    rho, xi, gamma, sigma, degenerate_tol are the reference's coefficients (defaults 1, 20, 0.1, 0.5, 1e-8).  mode="value"
    is DifferentiabilityMode::None (g comes back as zeros, no gradient test), mode="first" the reference on a First-mode
    function (value and gradient at the returned vertex, gradient test on).  The default stopping progress is the
    reference's for this solver: the conservative preset with x_delta_violations = 5."""
    _entry = "mi355_nelder_mead_minimize_batch"

    def __init__(self, stopping_progress=None, device=0, context=None, lanes_per_problem=0, dtype=None, **config):
        _float64_only(self, dtype)
        if stopping_progress is None:
            stopping_progress = capi.default_stop("conservative")   # nelder_mead.h:87-91
            stopping_progress.x_delta_violations = 5
        super().__init__(m=1, stopping_progress=stopping_progress, device=device, context=context,
                         arithmetic="exact", lanes_per_problem=lanes_per_problem)
        self.config = capi.default_nelder_mead_config(**config)

    def _desc(self, objective, n, per_problem=None, per_problem_stride=0):
        d = super()._desc(objective, n, per_problem, per_problem_stride)
        d.hessian_from_functor = 0
        d.hessian_diagonal = None
        d.hessian_condition = 0.0
        d.hessian_condition_stop = 0.0
        return d


class BatchedLbfgsb(BatchedLbfgs):
    """Batched `Lbfgsb<F, m>` (reference solver/lbfgsb.h, default m = 5; built for m <= 10): box-constrained L-BFGS-B.

    `SetBounds(lower, upper)` mirrors the reference (lbfgsb.h:89-93); without it the box is
    unbounded.  `SetBoundsPerProblem(lower, upper)` gives every problem of the batch its own box ([B, n] rows: what B
    reference solvers with B SetBounds calls solve; see mi355_lbfgsb_minimize_batch_boxes for the built range — at
    32 < n <= 64 arithmetic="default" is the reference-order kernel there).  stopping_progress defaults to what a
    default-constructed reference Lbfgsb uses (f_delta = 2.22e-9 relative on top of the default preset); its
    gradient_norm is the projected-gradient tolerance.  `minimize_callable(fn, x0)` minimises an objective the caller
    evaluates (torch ops, autograd) under the box in force — `LbfgsbAskTell`; n <= 64, m <= 8, reference-order arithmetic."""

    def __init__(self, m=5, stopping_progress=None, device=0, context=None, linesearch="more_thuente",
                 arithmetic="default", dtype=None):
        _float64_only(self, dtype)
        # arithmetic: "exact" = the reference-order kernels (lbfgsb_kernel.hpp, bit-identical to the oracle's butterfly
        # policy), "fma" = the relaxed-algebra kernels (lbfgsb_fast_kernel.hpp, bit-identical to their own CPU twin,
        # within 1e-6 of the reference), "default" = the library's choice (relaxed where it is built)
        super().__init__(m=m, linesearch=linesearch, arithmetic=arithmetic,
                         stopping_progress=stopping_progress or capi.default_stop("lbfgsb"),
                         device=device, context=context)
        self._lower = None
        self._upper = None
        self._rows = None    # SetBoundsPerProblem: (lower, upper), [B, n] each; in force while no shared box is set

    def SetBoundsPerProblem(self, lower, upper):
        """One box per problem: `lower` / `upper` are [B, n] float64 numpy arrays or tensors on the solver's device.
        `minimize` / `minimize_host` then check B and n against x0.  A later `SetBounds` returns to one shared box."""
        torch = self._torch
        rows = []
        for t in (lower, upper):
            if not torch.is_tensor(t):
                t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64))
            if t.dtype != torch.float64 or t.dim() != 2:
                raise ValueError("per-problem bounds must be [B, n] float64 arrays")
            if bool(torch.isnan(t).any()):
                raise ValueError("NaN bound (the breakpoint order of the Cauchy search would be undefined, as in the reference)")
            rows.append(t.to(self.device).contiguous())
        if rows[0].shape != rows[1].shape:
            raise ValueError("lower is %s, upper is %s" % (tuple(rows[0].shape), tuple(rows[1].shape)))
        self._rows = tuple(rows)
        self._lower = self._upper = None

    def _own_boxes(self, B, n):
        """The rows in force for a [B, n] batch, or None under a shared (or the default) box."""
        if self._rows is None or self._lower is not None:
            return None
        if tuple(self._rows[0].shape) != (B, n):
            raise ValueError("per-problem bounds are %s, x0 is %s" % (tuple(self._rows[0].shape), (B, n)))
        return self._rows

    def SetBounds(self, lower, upper):
        if np.isnan(np.asarray(lower, dtype=np.float64)).any() or np.isnan(np.asarray(upper, dtype=np.float64)).any():
            raise ValueError("NaN bound (the breakpoint order of the Cauchy search would be undefined, as in the reference)")
        torch = self._torch
        self._lower = torch.as_tensor(np.ascontiguousarray(lower, dtype=np.float64)).to(self.device)
        self._upper = torch.as_tensor(np.ascontiguousarray(upper, dtype=np.float64)).to(self.device)

    def minimize(self, objective, x0, want_gradient=True, want_progress=True, per_problem=None, trace=None):
        torch = self._torch
        if x0.dtype != torch.float64 or x0.dim() != 2 or not x0.is_cuda:
            raise ValueError("x0 must be a [B, n] float64 CUDA tensor")
        self._on_device(x0, "x0")
        x0 = x0.contiguous()
        B, n = x0.shape
        if self._lower is not None and self._lower.numel() != n:
            raise ValueError("bounds have %d entries, problems have %d" % (self._lower.numel(), n))
        x = torch.empty_like(x0)
        f = torch.empty(B, dtype=torch.float64, device=x0.device)
        g = torch.empty_like(x0) if want_gradient else None
        prog = torch.empty(B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=x0.device) \
            if want_progress else None
        d = self._desc(objective, n, *self._pp_device(per_problem, B))
        if trace is not None:
            self._trace_keepalive = trace
            d.trace = trace.c_pointer()
        rows = self._own_boxes(B, n)
        if rows is not None:
            capi.check(self.ctx._lib.mi355_lbfgsb_minimize_batch_boxes(
                self.ctx.handle, C.byref(d), rows[0].data_ptr(), rows[1].data_ptr(), n,
                B, x0.data_ptr(), x.data_ptr(), f.data_ptr(),
                g.data_ptr() if g is not None else None, prog.data_ptr() if prog is not None else None,
                self._stream()))
            return x, f, g, prog
        capi.check(self.ctx._lib.mi355_lbfgsb_minimize_batch(
            self.ctx.handle, C.byref(d),
            self._lower.data_ptr() if self._lower is not None else None,
            self._upper.data_ptr() if self._upper is not None else None,
            B, x0.data_ptr(), x.data_ptr(), f.data_ptr(),
            g.data_ptr() if g is not None else None, prog.data_ptr() if prog is not None else None,
            self._stream()))
        return x, f, g, prog

    def minimize_host(self, objective, x0, per_problem=None):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B, n = x0.shape
        x = np.empty_like(x0)
        g = np.empty_like(x0)
        f = np.empty(B)
        prog = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
        d = self._desc(objective, n)
        rows = self._own_boxes(B, n)
        if rows is not None:
            if per_problem is not None:
                pp = np.ascontiguousarray(per_problem, dtype=np.float64)
                d = self._desc(objective, n, pp.ctypes.data, pp.shape[1])
            lo, hi = (np.ascontiguousarray(t.cpu().numpy()) for t in rows)
            capi.check(self.ctx._lib.mi355_lbfgsb_minimize_batch_boxes_host(
                self.ctx.handle, C.byref(d), lo.ctypes.data, hi.ctypes.data, n, B, x0.ctypes.data, x.ctypes.data,
                f.ctypes.data, g.ctypes.data, prog.ctypes.data))
            return x, f, g, prog
        lo = self._lower.cpu().numpy() if self._lower is not None else None
        hi = self._upper.cpu().numpy() if self._upper is not None else None
        capi.check(self.ctx._lib.mi355_lbfgsb_minimize_batch_host(
            self.ctx.handle, C.byref(d), lo.ctypes.data if lo is not None else None,
            hi.ctypes.data if hi is not None else None, B, x0.ctypes.data, x.ctypes.data, f.ctypes.data,
            g.ctypes.data, prog.ctypes.data))
        return x, f, g, prog

    def _ask_tell(self, x0):
        return LbfgsbAskTell(self, x0)


class LbfgsbAskTell(LbfgsAskTell):
    """One ask/tell solve of `Lbfgsb<F, m, MoreThuente>::Minimize` (mi355_lbfgsb_ask_tell_*): B box-constrained problems
    whose objective the caller evaluates — the batched counterpart of scipy's L-BFGS-B with a loss written in torch.

        box = amd.BatchedLbfgsb(m=5); box.SetBounds(lower, upper)        # or SetBoundsPerProblem, or no box at all
        at = amd.LbfgsbAskTell(box, x0)
        while at.tell(*my_value_and_gradient(at.x)) > 0:
            pass
        x, f, g, progress = at.results()

    The protocol, `.x`, `tell`, `active`, `results` and `close` are LbfgsAskTell's.  The box in force on the solver is
    copied at creation.  `.asks`: how many problems asked for each kind of evaluation so far.  Built for n <= 64, m <= 8,
    the More-Thuente search and the reference-order arithmetic (arithmetic="default" is that here; "fma" is refused)."""
    _prefix = "mi355_lbfgsb_ask_tell_"
    _listed_suffix = "lbfgsb"
    ASK_KINDS = ("clip_start", "trial", "cauchy", "clip_next", "first")

    def _check_solver(self, solver):
        if type(solver) is not BatchedLbfgsb:
            raise TypeError("LbfgsbAskTell takes a BatchedLbfgsb (BatchedLbfgs has LbfgsAskTell)")

    def _create(self, solver, d, x0, h):
        rows = solver._own_boxes(self.B, self.n)
        if rows is not None:
            lower, upper, stride = rows[0], rows[1], self.n
        else:
            lower, upper, stride = solver._lower, solver._upper, 0
            if lower is not None and lower.numel() != self.n:
                raise ValueError("bounds have %d entries, problems have %d" % (lower.numel(), self.n))
        self._call("create", solver.ctx.handle, C.byref(d), lower.data_ptr() if lower is not None else None,
                   upper.data_ptr() if upper is not None else None, stride, self.B, x0.data_ptr(), solver._stream(),
                   C.byref(h))

    @property
    def asks(self):
        """{kind: count} over "clip_start", "trial", "cauchy", "clip_next", "first" (waits for the stream); once every
        problem has finished the counts add up to the sum of nfev."""
        if self._h is None:
            raise RuntimeError("this %s is closed" % type(self).__name__)
        counts = (C.c_int64 * len(self.ASK_KINDS))()
        self._call("asks", self._h, counts, self.solver._stream())
        return dict(zip(self.ASK_KINDS, (int(v) for v in counts)))


class DeviceGroup:
    """mi355_lbfgs_group: one engine context per entry of `devices` plus an RCCL communicator over the distinct devices.
    `minimize_host` shards a host batch into contiguous ranges, one host thread per member, and returns the
    all-reduced convergence record (problems, unconverged, iterations) — the path's only collective."""

    def __init__(self, devices):
        self._lib = capi.load()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        capi.check(self._lib.mi355_lbfgs_group_create(devs, len(devices), C.byref(h)))
        self._h = h
        self.devices = [int(d) for d in devices]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi355_lbfgs_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(self._lib.mi355_lbfgs_group_size(self._h))

    def minimize_host(self, solver, objective, x0, per_problem=None):
        """`solver`: a BatchedLbfgs carrying m / stopping / line search / arithmetic (its own context is not used)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B, n = x0.shape
        pp_ptr, pp_stride = None, 0
        if per_problem is not None:
            pp = np.ascontiguousarray(per_problem, dtype=np.float64)
            pp_ptr, pp_stride = pp.ctypes.data, pp.shape[1]
        x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
        prog = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
        flag = np.zeros(3, dtype=np.uint64)
        d = solver._desc(objective, n, pp_ptr, pp_stride)
        capi.check(self._lib.mi355_lbfgs_group_minimize_batch_host(
            self._h, C.byref(d), B, x0.ctypes.data, x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data,
            flag.ctypes.data))
        return x, f, g, prog, {"total": int(flag[0]), "unconverged": int(flag[1]), "iterations": int(flag[2]),
                               "all_converged": int(flag[1]) == 0}


    def _host_call(self, entry, solver, objective, x0, per_problem, extra=()):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B, n = x0.shape
        pp_ptr, pp_stride = None, 0
        if per_problem is not None:
            pp = np.ascontiguousarray(per_problem, dtype=np.float64)
            pp_ptr, pp_stride = pp.ctypes.data, pp.shape[1]
        x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
        prog = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
        flag = np.zeros(3, dtype=np.uint64)
        d = solver._desc(objective, n, pp_ptr, pp_stride)
        capi.check(getattr(self._lib, entry)(self._h, C.byref(d), *extra, B, x0.ctypes.data, x.ctypes.data, f.ctypes.data,
                                             g.ctypes.data, prog.ctypes.data, flag.ctypes.data))
        return x, f, g, prog, self._flag(flag)

    @staticmethod
    def _flag(flag):
        return {"total": int(flag[0]), "unconverged": int(flag[1]), "iterations": int(flag[2]),
                "all_converged": int(flag[1]) == 0}

    def minimize_host_lbfgsb(self, solver, objective, x0, lower=None, upper=None, per_problem=None):
        """mi355_lbfgsb_group_minimize_batch_host: `solver` a BatchedLbfgsb (m / stopping / arithmetic)."""
        if getattr(solver, "_rows", None) is not None and solver._lower is None:
            raise capi.EngineError(capi.ERR_UNSUPPORTED, "per-problem bounds (SetBoundsPerProblem) are not built for device "
                                                         "groups: one context, n <= 64")
        lo = np.ascontiguousarray(lower, dtype=np.float64) if lower is not None else None
        hi = np.ascontiguousarray(upper, dtype=np.float64) if upper is not None else None
        return self._host_call("mi355_lbfgsb_group_minimize_batch_host", solver, objective, x0, per_problem,
                               (lo.ctypes.data if lo is not None else None, hi.ctypes.data if hi is not None else None))

    def minimize_host_bfgs(self, solver, objective, x0, per_problem=None):
        return self._host_call("mi355_bfgs_group_minimize_batch_host", solver, objective, x0, per_problem)

    def minimize_device(self, solver, objective, x0_shards, lower=None, upper=None, per_problem_shards=None):
        """Device-resident sharded solve (mi355_lbfgs_group_minimize_batch / mi355_lbfgsb_group_minimize_batch):
        x0_shards[s] is a [B_s, n] float64 CUDA tensor on member s's device; lower / upper (host arrays) select Lbfgsb.
        Returns per-member (x, f, g, progress) tensors and the all-reduced convergence record."""
        import torch
        G = self.size()
        if len(x0_shards) != G:
            raise ValueError("one shard per group member")
        n = int(x0_shards[0].shape[1])
        outs, keep = [], []
        ptr = lambda ts: (C.c_void_p * G)(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])
        for s, x0 in enumerate(x0_shards):
            if x0.dtype != torch.float64 or x0.dim() != 2 or not x0.is_cuda or int(x0.shape[1]) != n:
                raise ValueError("shards must be [B_s, %d] float64 CUDA tensors" % n)
            x0_shards[s] = x0.contiguous()
            Bs = int(x0.shape[0])
            outs.append((torch.empty_like(x0), torch.empty(Bs, dtype=torch.float64, device=x0.device), torch.empty_like(x0),
                         torch.zeros(max(Bs, 1) * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=x0.device)))
        counts = (C.c_int64 * G)(*[int(t.shape[0]) for t in x0_shards])
        pps = None
        d = solver._desc(objective, n)
        if per_problem_shards is not None:
            pps = [p.contiguous() for p in per_problem_shards]
            d.per_problem_stride = int(pps[0].shape[1])
        flag = np.zeros(3, dtype=np.uint64)
        args = [counts, ptr(x0_shards), ptr([o[0] for o in outs]), ptr([o[1] for o in outs]), ptr([o[2] for o in outs]),
                ptr([o[3] for o in outs]), ptr(pps) if pps is not None else None, flag.ctypes.data]
        for t in x0_shards:                      # inputs produced on torch's streams must be complete
            torch.cuda.synchronize(t.device)
        if lower is not None:
            for t in x0_shards:
                keep.append((torch.as_tensor(np.ascontiguousarray(lower, dtype=np.float64)).to(t.device),
                             torch.as_tensor(np.ascontiguousarray(upper, dtype=np.float64)).to(t.device)))
                torch.cuda.synchronize(t.device)
            capi.check(self._lib.mi355_lbfgsb_group_minimize_batch(self._h, C.byref(d), ptr([k[0] for k in keep]),
                                                                   ptr([k[1] for k in keep]), *args))
        elif getattr(solver, "_entry", "") == "mi355_lbfgsb_minimize_batch" or isinstance(solver, BatchedLbfgsb):
            capi.check(self._lib.mi355_lbfgsb_group_minimize_batch(self._h, C.byref(d), None, None, *args))
        else:
            capi.check(self._lib.mi355_lbfgs_group_minimize_batch(self._h, C.byref(d), *args))
        return outs, self._flag(flag)


class ConstrainedProblem:
    """`ConstrainedOptimizationProblem` (function_problem.h:44-74) over the device term menu.

    Terms are built with `ConstrainedProblem.term`: a primitive (kind in capi.AL_TERM, or the id of a user term functor
    compiled into the library: MI355_AL_TERM_USER; `a` the coefficient vector of
    the linear / diagonal-quadratic kinds, `c` the constant of the diagonal quadratic) or a sum of primitives, entering
    as form in capi.AL_FORM ("plain" F, "value_minus_k" F - k, "k_minus_value" k - F).  `inequality` constraints
    mean g(x) >= 0, as in the reference.
    """

    @staticmethod
    def term(kind, form="plain", k=0.0, a=None, c=0.0, product=False):
        """One primitive (kind, a, c) as a term, or — `kind` a list of (kind, a, c) tuples — the sum F1 + F2 + ... of
        several (the reference's AddExpression, left to right); product=True with two tuples: their product F1 * F2
        (the reference's ProdExpression, function_expressions.h:260-315)."""
        prims = kind if isinstance(kind, (list, tuple)) else [(kind, a, c)]
        if product and len(prims) != 2:
            raise ValueError("a product term has exactly two primitives")
        return ([(p[0], p[1] if len(p) > 1 else None, float(p[2]) if len(p) > 2 else 0.0) for p in prims], form, float(k),
                bool(product))

    def __init__(self, n, objective, equality=(), inequality=(), user_params=None, family_equality=None,
                 family_inequality=None):
        # user_params: the blob handed to the user term functors that declare kTermParamsFromProblem (the parameters
        # the same functor takes as an objective; mi355_al_problem.user_params)
        self.user_params = None if user_params is None else np.ascontiguousarray(user_params, dtype=np.float64).ravel()
        # constraint FAMILIES (mi355_al_problem.family_eq / family_ineq): (A [F, n], k [F]) stands for the F affine
        # constraints A[i] . x - k[i] (= 0 / >= 0) — what a reference program pushes one `LinearFunctor(a_i) - k_i` at a
        # time into its constraint vectors (src/examples/svm_primal_al.cc:139-147); they follow the table's terms of
        # their kind in the problem's constraint order (and in lambda / mu)

        def family(pair):
            if pair is None:
                return np.zeros((0, int(n) + 1))
            A, k = np.asarray(pair[0], dtype=np.float64), np.asarray(pair[1], dtype=np.float64).ravel()
            if A.ndim != 2 or A.shape != (k.size, int(n)):
                raise ValueError("a constraint family is (A [F, n], k [F])")
            return np.ascontiguousarray(np.concatenate([A, k[:, None]], axis=1))

        self.family_eq, self.family_ineq = family(family_equality), family(family_inequality)
        terms = [objective] + list(equality) + list(inequality)
        if len(equality) > capi.AL_MAX_CONSTRAINTS or len(inequality) > capi.AL_MAX_CONSTRAINTS:
            raise ValueError("at most %d constraints of each kind" % capi.AL_MAX_CONSTRAINTS)
        prims = [p for t in terms for p in t[0]]
        if len(prims) > capi.AL_MAX_ROWS:
            raise ValueError("at most %d primitives" % capi.AL_MAX_ROWS)
        self.n, self.n_eq, self.n_ineq = int(n), len(equality), len(inequality)
        self.parts = np.array([capi.AL_PARTS_PRODUCT if (len(t) > 3 and t[3]) else len(t[0]) for t in terms], dtype=np.int32)
        # a primitive's kind: a name of the menu, or the objective id (>= capi.AL_TERM_USER) of a user term functor
        self.kinds = np.array([p[0] if isinstance(p[0], (int, np.integer)) else capi.AL_TERM[p[0]] for p in prims],
                              dtype=np.int32)
        self.forms = np.array([capi.AL_FORM[t[1]] for t in terms], dtype=np.int32)
        self.ks = np.array([t[2] for t in terms], dtype=np.float64)
        self.coef = np.zeros((len(prims), self.n + 1))
        for i, p in enumerate(prims):
            if p[1] is not None:
                self.coef[i, :self.n] = np.asarray(p[1], dtype=np.float64)
            self.coef[i, self.n] = p[2]

    def c_struct(self):
        p = capi.AlProblem()
        p.n, p.n_eq, p.n_ineq = self.n, self.n_eq, self.n_ineq
        p.kinds = self.kinds.ctypes.data_as(C.POINTER(C.c_int32))
        p.forms = self.forms.ctypes.data_as(C.POINTER(C.c_int32))
        p.ks = self.ks.ctypes.data_as(C.POINTER(C.c_double))
        p.coef = self.coef.ctypes.data_as(C.POINTER(C.c_double))
        p.parts = self.parts.ctypes.data_as(C.POINTER(C.c_int32))
        if self.user_params is not None and self.user_params.size:
            p.user_params = self.user_params.ctypes.data_as(C.POINTER(C.c_double))
            p.user_params_count = int(self.user_params.size)
        p.n_family_eq, p.n_family_ineq = self.family_eq.shape[0], self.family_ineq.shape[0]
        if p.n_family_eq:
            p.family_eq = self.family_eq.ctypes.data_as(C.POINTER(C.c_double))
        if p.n_family_ineq:
            p.family_ineq = self.family_ineq.ctypes.data_as(C.POINTER(C.c_double))
        return p

    @property
    def n_eq_all(self):     # width of lambda: the table's equalities, then the family's
        return self.n_eq + self.family_eq.shape[0]

    @property
    def n_ineq_all(self):   # width of mu
        return self.n_ineq + self.family_ineq.shape[0]


def AugLagComposite(problem):
    """`ToAugmentedLagrangian(problem, multipliers, penalty)` (function_penalty.h:239-246) as an objective for
    BatchedLbfgs: pass the rows (lambda, mu, penalty) as `per_problem=` of minimize / minimize_host.

    The composite objective (MI355_OBJ_AL_COMPOSITE) is described by the term TABLE only; a problem that also carries
    constraint families (family_equality / family_inequality) is refused — silently dropping them would hand the caller
    the value and gradient of a different function (round-5 advisor finding)."""
    if problem.family_eq.shape[0] or problem.family_ineq.shape[0]:
        raise ValueError("AugLagComposite: the problem carries constraint families (%d equalities, %d inequalities); the "
                         "composite objective holds table terms only — solve it with BatchedAugmentedLagrangian"
                         % (problem.family_eq.shape[0], problem.family_ineq.shape[0]))
    terms = np.column_stack([problem.parts.astype(np.float64), problem.forms.astype(np.float64), problem.ks])
    rows = np.concatenate([problem.kinds[:, None].astype(np.float64), problem.coef], axis=1)
    head = [float(problem.n_eq), float(problem.n_ineq), float(len(problem.kinds))]
    return Objective(capi.OBJ_AL_COMPOSITE, np.concatenate([head, terms.ravel(), rows.ravel()]), "al_composite")


class BatchedAugmentedLagrangian:
    """Batched `AugmentedLagrangian<Problem, Lbfgs<FunctionExpr, m>>` (solver/augmented_lagrangian.h).

    config: capi.AlConfig (default: the reference's AugmentedLagrangianConfig and constrained stopping defaults);
    inner_stopping_progress: the inner solver's stopping_progress (default DefaultStoppingSolverProgress).
    """

    def __init__(self, m=None, config=None, inner_stopping_progress=None, device=0, context=None,
                 linesearch="more_thuente", inner="lbfgs", lower=None, upper=None):
        # inner="lbfgsb": Lbfgsb<F, m> (default m = 5) as the inner solver, `lower` / `upper` its SetBounds box (n
        # doubles each, or None = never set); its default stopping test is the Lbfgsb constructor's
        if inner not in ("lbfgs", "lbfgsb"):
            raise ValueError("inner must be 'lbfgs' or 'lbfgsb'")
        self.box = inner == "lbfgsb"
        if (lower is None) != (upper is None) or (lower is not None and not self.box):
            raise ValueError("lower / upper come together and need inner='lbfgsb'")
        self.lower = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64)
        if m is None:
            m = 5 if self.box else 10
        self.m = int(m)
        # the LineSearch template argument of the inner Lbfgs (lbfgs.h:41)
        self.linesearch = {"more_thuente": capi.LS_MORE_THUENTE, "hager_zhang": capi.LS_HAGER_ZHANG}[linesearch]
        self.ctx = context or Context(device)
        self.config = config or self.default_config()
        self.inner_stopping_progress = inner_stopping_progress or capi.default_stop()
        if self.box and inner_stopping_progress is None:  # Lbfgsb(): f_delta = 2.22e-9, relative (lbfgsb.h:84-87)
            self.inner_stopping_progress.f_delta = 2.22e-9
            self.inner_stopping_progress.f_delta_relative = 1

    def _bounds(self, n):
        if self.lower is None:
            return None, None
        if self.lower.shape != (n,) or self.upper.shape != (n,):
            raise ValueError("lower / upper must hold n entries")
        return self.lower.ctypes.data, self.upper.ctypes.data

    def default_config(self, **overrides):
        c = capi.AlConfig()
        capi.check(self.ctx._lib.mi355_auglag_default_config(C.byref(c)))
        for k, v in overrides.items():
            setattr(c, k, v)
        return c

    @staticmethod
    def _state(problem, x0, lambda0, mu0, penalty0):
        x = np.array(x0, dtype=np.float64, order="C", ndmin=2)
        B = x.shape[0]

        def rows(v, width):
            if width == 0:
                return np.zeros((B, 0))
            v = np.zeros((B, width)) if v is None else np.asarray(v, dtype=np.float64)
            return np.ascontiguousarray(np.broadcast_to(v.reshape(-1, width) if v.ndim else v, (B, width)).copy())

        pen = np.ascontiguousarray(np.broadcast_to(np.asarray(penalty0, dtype=np.float64), (B,)).copy())
        return x, rows(lambda0, problem.n_eq_all), rows(mu0, problem.n_ineq_all), pen

    @staticmethod
    def _constants(problem, term_constants, B):
        if term_constants is None:
            return None
        tc = np.ascontiguousarray(term_constants, dtype=np.float64)
        if tc.shape != (B, 1 + problem.n_eq + problem.n_ineq):
            raise ValueError("term_constants must be [B, 1 + n_eq + n_ineq]")
        return tc

    def minimize_host(self, problem, x0, lambda0=None, mu0=None, penalty0=0.0, term_constants=None, max_violation0=0.0):
        """numpy in, dict of numpy out (x, lambda, mu, penalty, max_violation, max_lagrangian_gradient, progress).
        term_constants [B, 1 + n_eq + n_ineq]: row b replaces the constants k of the problem's terms, so the batch
        is B different problems of one shape rather than B starts of one problem."""
        x, lam, mu, pen = self._state(problem, x0, lambda0, mu0, penalty0)
        B = x.shape[0]
        tc = self._constants(problem, term_constants, B)
        # max_violation is in/out: the incoming state's value (0 for a fresh state) feeds the first penalty-growth test
        viol = np.ascontiguousarray(np.broadcast_to(np.asarray(max_violation0, dtype=np.float64), (B,)).copy())
        kkt = np.empty(B)
        prog = np.zeros(B, dtype=capi.AL_PROGRESS_DTYPE)
        ps = problem.c_struct()
        head = (self.ctx.handle, C.byref(ps), C.byref(self.config), C.byref(self.inner_stopping_progress), self.m,
                self.linesearch)
        tail = (B, tc.ctypes.data if tc is not None else None, x.ctypes.data, lam.ctypes.data if lam.size else None,
                mu.ctypes.data if mu.size else None, pen.ctypes.data, viol.ctypes.data, kkt.ctypes.data,
                prog.ctypes.data)
        if self.box:
            capi.check(self.ctx._lib.mi355_auglag_box_minimize_batch_host(*head, *self._bounds(problem.n), *tail))
        else:
            capi.check(self.ctx._lib.mi355_auglag_minimize_batch_host(*head, *tail))
        return {"x": x, "lambda": lam, "mu": mu, "penalty": pen, "max_violation": viol,
                "max_lagrangian_gradient": kkt, "progress": prog}

    def minimize(self, problem, x, lam, mu, penalty, term_constants=None, max_violation=None):
        """Device tensors, updated in place: x [B, n], lam [B, n_eq (+ family)], mu [B, n_ineq (+ family)], penalty [B] (float64, CUDA);
        term_constants: optional [B, 1 + n_eq + n_ineq] device tensor (see minimize_host).
        Returns (max_violation, max_lagrangian_gradient, progress bytes) as device tensors."""
        import torch
        B = x.shape[0]
        if term_constants is not None and tuple(term_constants.shape) != (B, 1 + problem.n_eq + problem.n_ineq):
            raise ValueError("term_constants must be [B, 1 + n_eq + n_ineq]")
        for t in (x, lam, mu, penalty, term_constants):
            if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("state tensors must be contiguous float64 CUDA tensors")
        # in/out: the incoming states' max_violation (a tensor returned by an earlier call), zeros for fresh states
        viol = max_violation if max_violation is not None else torch.zeros(B, dtype=torch.float64, device=x.device)
        kkt = torch.empty_like(viol)
        prog = torch.empty(B * capi.AL_PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=x.device)
        ps = problem.c_struct()
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        head = (self.ctx.handle, C.byref(ps), C.byref(self.config), C.byref(self.inner_stopping_progress), self.m,
                self.linesearch)
        tail = (B, term_constants.data_ptr() if term_constants is not None else None, x.data_ptr(),
                lam.data_ptr() if problem.n_eq_all else None, mu.data_ptr() if problem.n_ineq_all else None,
                penalty.data_ptr(), viol.data_ptr(), kkt.data_ptr(), prog.data_ptr(), stream)
        if self.box:
            capi.check(self.ctx._lib.mi355_auglag_box_minimize_batch(*head, *self._bounds(problem.n), *tail))
        else:
            capi.check(self.ctx._lib.mi355_auglag_minimize_batch(*head, *tail))
        return viol, kkt, prog

    def last_launch(self):
        """The dict of BatchedLbfgs.last_launch(): the record of the most recent launch of the inner-solver kernel on this
        solver's context — the one launch of the fused loop; in the lock-step loop the last inner launch (after a
        hand-over: the fused launch that took the survivors)."""
        return BatchedLbfgs.last_launch(self)

    def evaluate_host(self, problem, x, lam=None, mu=None, penalty=0.0, term_constants=None):
        """Value and gradient of ToAugmentedLagrangian(problem, (lam, mu), penalty) at every row of x."""
        x, lam, mu, pen = self._state(problem, x, lam, mu, penalty)
        B = x.shape[0]
        tc = self._constants(problem, term_constants, B)
        f, g = np.empty(B), np.empty_like(x)
        ps = problem.c_struct()
        capi.check(self.ctx._lib.mi355_auglag_eval_batch_host(
            self.ctx.handle, C.byref(ps), B, tc.ctypes.data if tc is not None else None, x.ctypes.data,
            lam.ctypes.data if lam.size else None,
            mu.ctypes.data if mu.size else None, pen.ctypes.data, f.ctypes.data, g.ctypes.data))
        return f, g


@dataclass
class DerivativeCheck:
    """What check_derivatives returns: device tensors.  f [B], grad / grad_fd [B, n] (the functor's gradient, the
    finite-difference one), hess / hess_fd [B, n, n] (entry [b, j, i] is H(i, j): column major, as hess_full writes it;
    None without hessian=True) and the fields of mi355_derivative_report as [B] tensors."""
    f: object
    grad: object
    grad_fd: object
    hess: object
    hess_fd: object
    gradient_ok: object
    hessian_ok: object
    gradient_worst_index: object
    hessian_worst_index: object
    nonfinite: object
    gradient_worst_excess: object
    hessian_worst_excess: object
    report: object   # the raw records: uint8 [B * 40], capi.DERIVATIVE_REPORT_DTYPE


def check_derivatives(objective, x, *, hessian=True, accuracy=3, gradient_step=0.0, hessian_step=0.0,
                      gradient_tolerance=0.0, hessian_tolerance=0.0, lanes_per_problem=0, context=None):
    """The reference's IsGradientCorrect / IsHessianCorrect (utils/derivatives.h) on the DEVICE functor of `objective`
    at every row of x ([B, n] float64 CUDA tensor): mi355_check_derivatives_batch.  Steps and tolerances of 0 are the
    reference's (h = 2^-26 max(|x_d|, 1), 1e-2f, 1e-1f); hessian_step=2**-13 makes the Hessian check usable away from
    a minimiser, where the reference's step drowns the second difference in rounding noise.
    Asynchronous on the current stream.  Returns a DerivativeCheck."""
    import torch
    if x.dtype != torch.float64 or x.dim() != 2 or not x.is_cuda:
        raise ValueError("x must be a [B, n] float64 CUDA tensor")
    ctx = context or Context(x.device.index or 0)
    if x.device != torch.device("cuda", ctx.device):
        raise ValueError("x lives on %s, the context on cuda:%d" % (x.device, ctx.device))
    x = x.contiguous()
    B, n = x.shape
    d = capi.Desc()
    d.objective = objective.objective_id
    d.n = int(n)
    d.m = 1
    p = np.ascontiguousarray(objective.params, dtype=np.float64)
    d.objective_params = p.ctypes.data_as(C.POINTER(C.c_double)) if p.size else None
    d.n_params = int(p.size)
    d.lanes_per_problem = int(lanes_per_problem)
    c = capi.DerivativeConfig(int(accuracy), int(accuracy), float(gradient_step), float(hessian_step),
                              float(gradient_tolerance), float(hessian_tolerance))
    f = torch.empty(B, dtype=torch.float64, device=x.device)
    grad, grad_fd = torch.empty_like(x), torch.empty_like(x)
    hess = torch.empty(B, n, n, dtype=torch.float64, device=x.device) if hessian else None
    hess_fd = torch.empty_like(hess) if hessian else None
    report = torch.empty(B * capi.DERIVATIVE_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=x.device)
    capi.check(ctx._lib.mi355_check_derivatives_batch(
        ctx.handle, C.byref(d), C.byref(c), B, x.data_ptr(), f.data_ptr(), grad.data_ptr(), grad_fd.data_ptr(),
        hess.data_ptr() if hessian else None, hess_fd.data_ptr() if hessian else None, report.data_ptr(),
        C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    ints = report.view(torch.int32).view(B, 10)
    doubles = report.view(torch.float64).view(B, 5)
    out = DerivativeCheck(f, grad, grad_fd, hess, hess_fd, ints[:, 0], ints[:, 1], ints[:, 2], ints[:, 3], ints[:, 4],
                          doubles[:, 3], doubles[:, 4], report)
    out._keepalive = (p, ctx)   # (the call is asynchronous: the blob and a context made here outlive it with the result)
    return out


def al_progress_to_numpy(prog):
    """Device progress bytes of BatchedAugmentedLagrangian.minimize -> numpy records (capi.AL_PROGRESS_DTYPE)."""
    return prog.cpu().numpy().view(capi.AL_PROGRESS_DTYPE)


def progress_to_numpy(prog):
    """Device uint8 progress buffer -> numpy record array (copies to host)."""
    return prog.cpu().numpy().view(capi.PROGRESS_DTYPE)


def _splitmix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _normal_from_counter(seed, idx):
    """N(0,1) from a counter: two splitmix64 uniforms -> Box-Muller (host only)."""
    a = _splitmix64(np.uint64(seed) ^ (idx * np.uint64(2)))
    b = _splitmix64(np.uint64(seed) ^ (idx * np.uint64(2) + np.uint64(1)))
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)  # (0, 1]
    u2 = (b >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def synthetic_ridge_host(B, rows=128, n=64, seed=20260923, first_problem=0):
    """Config-4 inputs: one shared A (rows x n) with N(0,1)/sqrt(rows)
    entries and one right-hand side y_b ~ N(0,1)^rows per problem; counter based, so shards of
    a global batch line up.  Returns (A, Y[B, rows])."""
    ia = np.arange(rows * n, dtype=np.uint64)
    A = (_normal_from_counter(seed ^ 0xA11CE, ia) / np.sqrt(float(rows))).reshape(rows, n)
    iy = (np.arange(first_problem, first_problem + B, dtype=np.uint64)[:, None] * np.uint64(rows)
          + np.arange(rows, dtype=np.uint64)[None, :])
    Y = _normal_from_counter(seed ^ 0xB0B, iy)
    return A, Y


def synthetic_x0_host(B, n, kind="std", seed=20260923, first_problem=0):
    """Host twin of mi355_lbfgs_fill_x0 (bit-identical), for CPU-side checks."""
    idx = (np.arange(first_problem, first_problem + B, dtype=np.uint64)[:, None] * np.uint64(n)
           + np.arange(n, dtype=np.uint64)[None, :])
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ idx
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    if kind == "std":
        base = np.where(np.arange(n) % 2 == 1, 1.0, -1.2)[None, :]
        return base + 0.1 * (2.0 * u - 1.0)
    return -2.0 + 4.0 * u
