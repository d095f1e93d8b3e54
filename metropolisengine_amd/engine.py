"""``MetropolisEngine``: the reference's class surface over N independent chains on one MI355X.

Mirrors ``metropolisengine.MetropolisEngine`` (the reference's metropolisengine/metropolis_engine.py:10-463):
same constructor arguments in the same order, ``step_all()`` / ``measure()``, the same attribute names.  All
arithmetic happens in libmetropolis_hip.so (HIP kernels, C ABI in include/metropolis_engine.h); this class only
marshals arguments and unpacks results.  Differences from the reference, all forced by the GPU setting:

 * ``energy_functions`` is an :class:`~metropolisengine_amd.energy.EnergySpec` (built-in energy or a hand-written HIP device
   function) OR, exactly as in the reference, a Python callable ``(real_params, complex_params) -> float`` / the dictionary of
   term callables: the callable is traced once on symbolic parameters and compiled into a plugin (``pyenergy.py``; hipcc, about a
   minute on first use, cached).  ``reject_condition`` is a :class:`~metropolisengine_amd.energy.RejectSpec` or, with a Python
   energy, a Python predicate.  (The reference silently drops a ``reject_condition`` given to the constructor -- SURVEY.md
   quirk Q6; here it is honoured.)
 * keyword-only extras: ``n_chains``, ``seed``, ``dtype``, ``device``, ``chain_offset``, ``cov_mode``, ``trace_chains``,
   ``trace_stride``, ``track_covariance``, ``reference_energy_ledgers`` (reproduce the reference's two energy ledgers,
   SURVEY.md quirk Q5: ``step_all`` of a mixed engine uses ``energy_total``, group steps ``energy[term]``).
 * ``temperatures=[T_0, ..., T_{K-1}]`` (keyword-only, with ``temp=0``): a temperature ladder -- K rungs of
   ``n_chains / K`` consecutive chains, rung k stepping at ``T_k`` -- and :meth:`replica_exchange` swaps between adjacent
   rungs (parallel tempering; no reference counterpart).
 * :meth:`set_temp` changes the scalar temperature of a running engine (simulated annealing); :meth:`resample` /
   :meth:`anneal` run population annealing -- Boltzmann resampling of the chains between temperatures, with the free-energy
   estimate ``ln Z(T_new) / Z(T_old)`` of every stage in :meth:`population_stats` (no reference counterpart).
 * with ``n_chains == 1`` attributes have the reference's shapes and ``step_all()`` returns a bool; with more
   chains they gain a leading chain axis and ``step_all()`` returns ``None`` (it stays asynchronous).
 * randomness is a seeded counter-based Philox stream per global chain id instead of numpy's global state.
 * parameter-space size: like the reference, no fixed limit on the number of parameters -- up to 96 real degrees of freedom
   (``n_real + 2 n_complex``) the register-resident kernels, up to 128 a kernel set compiled on first use for the default
   ``cov_mode="reference"``, beyond that the runtime-dimension kernels (identity shape or per-chain shapes for any space, one
   shared factor for pure real ones) as long as 64 x D values fit the LDS (float64: D <= 290); README.md "Limits".
"""
import ctypes

import numpy as np

from . import _capi
from .energy import EnergySpec, RejectSpec

_DTYPES = {"f32": _capi.ME_F32, "float32": _capi.ME_F32, "f64": _capi.ME_F64, "float64": _capi.ME_F64}
_COV_MODES = {"reference": _capi.COV_REFERENCE, "fixed": _capi.COV_FIXED, "pooled": _capi.COV_POOLED}


_as_double_ptr = _capi.double_ptr


def _initial_state(initial_real_params, initial_complex_params):
    """[real | Re z | Im z] of the initial parameters (one more state for the traced energy's self-check), or None if
    they do not convert; the constructor validates them itself."""
    try:
        r = np.asarray([] if initial_real_params is None else initial_real_params, dtype=np.float64).reshape(-1)
        c = np.asarray([] if initial_complex_params is None else initial_complex_params, dtype=np.complex128).reshape(-1)
    except (TypeError, ValueError):
        return None
    return np.concatenate([r, c.real, c.imag])


def unpack_real_block(packed, nr):
    """[n, P] packed lower triangles -> [n, nr, nr] symmetric matrices (real block of ME_FIELD_COV)."""
    n = packed.shape[0]
    out = np.zeros((n, nr, nr))
    il = np.tril_indices(nr)
    out[:, il[0], il[1]] = packed[:, :nr * (nr + 1) // 2]
    out[:, il[1], il[0]] = packed[:, :nr * (nr + 1) // 2]
    return out


def unpack_complex_block(packed, nr, nc, hermitian=True):
    """[n, P] -> [n, nc, nc] complex: Hermitian matrices (covariance) or lower-triangular factors."""
    n = packed.shape[0]
    pr = nr * (nr + 1) // 2
    out = np.zeros((n, nc, nc), dtype=np.complex128)
    for i in range(nc):
        for j in range(i):
            v = packed[:, pr + i * i + 2 * j] + 1j * packed[:, pr + i * i + 2 * j + 1]
            out[:, i, j] = v
            if hermitian:
                out[:, j, i] = np.conj(v)
        out[:, i, i] = packed[:, pr + i * i + 2 * i]
    return out


def unpack_real_factor(packed, nr):
    n = packed.shape[0]
    out = np.zeros((n, nr, nr))
    il = np.tril_indices(nr)
    out[:, il[0], il[1]] = packed[:, :nr * (nr + 1) // 2]
    return out


def validate_ladder(temperatures, n_chains):
    """A temperature ladder as a float64 array: ``T_0 < T_1 < ... < T_{K-1}``, finite and > 0, and ``n_chains`` a multiple
    of ``64 K`` (every rung is a run of whole 64-chain tiles).  Raises ``ValueError``."""
    temps = np.asarray(temperatures, dtype=np.float64)
    if temps.ndim != 1 or temps.size < 1:
        raise ValueError("temperatures must be a non-empty 1-D sequence")
    if not np.all(np.isfinite(temps)) or not np.all(temps > 0):
        raise ValueError("ladder temperatures must be finite and > 0")
    if not np.all(np.diff(temps) > 0):
        raise ValueError("ladder temperatures must be strictly increasing")
    if int(n_chains) % (64 * temps.size) != 0:
        raise ValueError("n_chains (%d) must be a multiple of 64 * %d rungs: every rung is a run of whole 64-chain tiles"
                         % (int(n_chains), temps.size))
    return temps


def set_cache_budget(n_bytes):
    """Process-wide tuning knob (``me_set_cache_budget``): launches whose working set exceeds ``n_bytes`` stream their
    read-once / write-once fields with the non-temporal cache policy.  Default 224 MiB."""
    _capi.check(_capi.load().me_set_cache_budget(int(n_bytes)))


class MetropolisEngine:
    def __init__(self, energy_functions, reject_condition=None, initial_real_params=None,
                 initial_complex_params=None, sampling_width=0.05, covariance_matrix_real=None,
                 covariance_matrix_complex=None, params_names=None, target_acceptance=.3, temp=0,
                 complex_sample_method="multivariate-gaussian", *, n_chains=1, seed=0, dtype="f32", device=0,
                 chain_offset=0, cov_mode="reference", trace_chains=None, trace_stride=1, track_covariance=False,
                 reference_energy_ledgers=False, temperatures=None):
        if initial_real_params is None and initial_complex_params is None:
            print("must give list containing  at least one value for initial real or complex parameters")
            raise ValueError("no initial parameters")                                    # metropolis_engine.py:37-39
        if temperatures is not None:
            # checked before anything is built or traced: a ladder replaces the scalar temp
            if temp is None or temp != 0:
                raise ValueError("give either temp or temperatures: a ladder engine steps every rung at its own temperature")
            temperatures = validate_ladder(temperatures, n_chains)
        if not isinstance(energy_functions, EnergySpec):
            # the reference's own form: a Python callable (real_params, complex_params) -> float, or its dictionary of
            # term callables (metropolis_engine.py:20, :111-116).  It is TRACED once on symbolic parameters, written out as
            # a HIP device function and compiled around the kernels (pyenergy.py) -- there is still no CPU fallback.
            if not (callable(energy_functions) or isinstance(energy_functions, dict)):
                raise TypeError("energy_functions must be an EnergySpec (IsoQuadratic, DiagQuadratic, DenseQuadratic, LandauToy, "
                                "CylinderSurrogate, UserEnergy), a callable (real_params, complex_params) -> float, or the "
                                "reference's dictionary of term callables")
            from .pyenergy import PythonEnergy, PythonReject
            traced_reject = reject_condition if (reject_condition is not None and not isinstance(reject_condition, RejectSpec)) else None
            if traced_reject is not None and not callable(traced_reject):
                raise TypeError("reject_condition must be a RejectSpec, a callable (real_params, complex_params) -> bool, or None")
            energy_functions = PythonEnergy(energy_functions, reject=traced_reject,
                                            initial=_initial_state(initial_real_params, initial_complex_params))
            if traced_reject is not None:
                reject_condition = PythonReject()
        if reject_condition is not None and not isinstance(reject_condition, RejectSpec):
            raise TypeError("reject_condition must be a metropolisengine_amd.energy.RejectSpec or None (a Python predicate is "
                            "accepted together with a Python energy: both are traced into one plugin)")
        if complex_sample_method not in ("magnitude-phase", "multivariate-gaussian"):
            print("complex_sample_method", complex_sample_method, "not recognized")       # :131-133
            print("defaulting to multivariate-gaussian")
        if temp is None or not temp >= 0:
            raise AssertionError("temp must be >= 0")                                     # :92
        if isinstance(sampling_width, (list, tuple)):
            # the reference accepts [real, complex] but then breaks in mixed engines (quirk Q7)
            if initial_real_params is not None and initial_complex_params is not None:
                raise ValueError("a [real, complex] sampling_width list is not usable with mixed parameter spaces")
            initial_widths = (float(sampling_width[0]), float(sampling_width[1]))               # :94-95
            sampling_width = sampling_width[0] if initial_real_params is not None else sampling_width[1]
        else:
            initial_widths = (float(sampling_width), float(sampling_width))                     # :97-99

        real0 = np.zeros(0) if initial_real_params is None else np.asarray(initial_real_params, dtype=np.float64).ravel()
        cplx0 = (np.zeros(0, dtype=np.complex128) if initial_complex_params is None
                 else np.asarray(initial_complex_params, dtype=np.complex128).ravel())
        self.num_real_params = int(real0.size)
        self.num_complex_params = int(cplx0.size)
        self.param_space_dims = self.num_real_params + self.num_complex_params          # :60
        nr, nc = self.num_real_params, self.num_complex_params
        self.n_chains = int(n_chains)
        self.dtype = dtype
        self.seed = int(seed)
        self.chain_offset = int(chain_offset)
        self.temp = temp
        self._population_used = False    # set_temp / resample were used: checkpoints then carry temp, stages and families
        self._initial_temp = temp        # what a checkpoint without "temp" describes
        self.target_acceptance = target_acceptance
        self._initial_widths = initial_widths     # what the width of an absent group stays at
        # "magnitude-phase" swaps step_complex_group only; step_all keeps the Gaussian sampler (:129-130, quirk Q9)
        self.complex_sample_method = ("magnitude-phase" if complex_sample_method == "magnitude-phase"
                                      else "multivariate-gaussian")
        self._energy_spec = energy_functions
        self._reject_spec = reject_condition
        if params_names:
            self.params_names = params_names                                             # :82-85
        else:
            self.params_names = ["param_" + str(i) for i in range(nr + nc)]
        self.observables_names = ["abs_param_" + str(i) for i in range(nr + nc)]        # :86-87
        self.observables_names.extend(["param_" + str(i) + "_squared" for i in range(nr)])
        self.energy_term_names = list(energy_functions.term_names)                       # :112-118
        self.df = None

        self._lib = _capi.load()
        coeffs = np.ascontiguousarray(energy_functions.coefficients(nr, nc), dtype=np.float64)
        init = np.ascontiguousarray(np.concatenate((real0, cplx0.real, cplx0.imag)), dtype=np.float64)
        cfg = _capi.MeConfig()
        cfg.abi_version = _capi.ABI_VERSION
        cfg.device_id = self.device = int(device)
        cfg.n_chains = self.n_chains
        cfg.chain_offset = self.chain_offset
        cfg.seed = self.seed
        cfg.n_real, cfg.n_complex = nr, nc
        if dtype not in _DTYPES:
            raise ValueError("dtype must be one of %s" % sorted(_DTYPES))
        cfg.dtype = _DTYPES[dtype]
        if cov_mode not in _COV_MODES:
            raise ValueError("cov_mode must be one of %s" % sorted(_COV_MODES))
        cfg.cov_mode = _COV_MODES[cov_mode]
        self.cov_mode = cov_mode
        # parameter spaces whose packed matrix is too large for registers (> 160 entries, e.g. 64 real parameters) keep
        # the per-chain matrices only where the proposals need them (cov_mode="reference": streamed kernels, pure real
        # spaces) or on request (track_covariance=True: statistics only)
        self.reference_energy_ledgers = bool(reference_energy_ledgers)
        cfg.flags = ((_capi.FLAG_TRACK_COVARIANCE if track_covariance else 0) |
                     (_capi.FLAG_REFERENCE_ENERGY_LEDGERS if reference_energy_ledgers else 0))
        cfg.temp = float(temp)
        cfg.target_acceptance = float(target_acceptance)
        cfg.sampling_width = float(sampling_width)
        cfg.energy_kind = energy_functions.kind
        if hasattr(energy_functions, "ensure_loaded"):          # UserEnergy: build + load its plugin library
            energy_functions.ensure_loaded(nr, nc)
            self._user_name = energy_functions.name.encode()
            cfg.user_energy_name = self._user_name
        cfg.n_energy_coeffs = int(coeffs.size)
        cfg.energy_coeffs = _as_double_ptr(coeffs)
        cfg.reject_kind = reject_condition.kind if reject_condition is not None else _capi.REJECT_NONE
        cfg.reject_bound = reject_condition.bound if reject_condition is not None else 0.0
        cfg.initial_params = _as_double_ptr(init)
        keep = [coeffs, init]
        if covariance_matrix_real is not None and nr:
            c_r = np.ascontiguousarray(covariance_matrix_real, dtype=np.float64)
            if c_r.shape != (nr, nr):
                raise ValueError("covariance_matrix_real must be %dx%d" % (nr, nr))
            cfg.covariance_real = _as_double_ptr(c_r)
            keep.append(c_r)
        if covariance_matrix_complex is not None and nc:
            c_c = np.asarray(covariance_matrix_complex, dtype=np.complex128)
            if c_c.shape != (nc, nc):
                raise ValueError("covariance_matrix_complex must be %dx%d" % (nc, nc))
            c_ri = np.ascontiguousarray(np.stack((c_c.real, c_c.imag), axis=-1), dtype=np.float64)
            cfg.covariance_complex = _as_double_ptr(c_ri)
            keep.append(c_ri)
        handle = ctypes.c_void_p()
        self._handle = None
        if not hasattr(energy_functions, "ensure_loaded"):
            from . import build
            d = nr + 2 * nc
            if not self._lib.me_supported(cfg.dtype, nr, nc, _capi.ENERGY_ISO_QUAD):
                # dimensions outside the prebuilt set: compile this (nr, nc) kernel set once (hipcc) and load it
                _capi.check(self._lib.me_load_plugin(build.build_dims(nr, nc).encode()))
            elif build.MAX_REGISTER_DOF < d <= build.MAX_COMPILED_DOF and cov_mode == "reference":
                # beyond 96 degrees of freedom the runtime-dimension set (no build) has per-chain shapes too, slower ones per
                # step: up to MAX_COMPILED_DOF the space's own kernel set is compiled after all for the reference's
                # semantics (streamed shapes; minutes of hipcc, cached)
                _capi.check(self._lib.me_load_plugin(build.build_dims(nr, nc).encode()))
        _capi.check(self._lib.me_create(ctypes.byref(cfg), ctypes.byref(handle)))
        self._handle = handle
        n_terms = ctypes.c_int32()
        _capi.check(self._lib.me_energy_terms(handle, ctypes.byref(n_terms)), handle)
        if n_terms.value != len(self.energy_term_names):
            raise ValueError("the energy has %d terms on the device but term_names=%r" %
                             (n_terms.value, tuple(self.energy_term_names)))
        alpha, ratio, m = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
        _capi.check(self._lib.me_constants(handle, ctypes.byref(alpha), ctypes.byref(m), ctypes.byref(ratio)), handle)
        self.alpha, self.m, self.ratio = alpha.value, m.value, ratio.value               # :101-107
        self._last_accepted = 0
        # time series (:31-35, :350-356): the reference records its one chain at every measure(); a single-chain engine
        # does the same, a many-chain engine records ``trace_chains`` chains (every ``trace_stride``-th) on request
        self.trace_chains = (1 if self.n_chains == 1 else 0) if trace_chains is None else int(trace_chains)
        self.trace_stride = int(trace_stride)
        if self.trace_chains:
            _capi.check(self._lib.me_trace_enable(handle, self.trace_chains, self.trace_stride), handle)
        if temperatures is not None:
            self.set_temperatures(temperatures)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._lib.me_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        _capi.check(status, self._handle)

    # ------------------------------------------------------------------ stepping (metropolis_engine.py:209-259)
    def step_all(self, n_sweeps=1):
        """One (or ``n_sweeps`` fused) propose -> energy -> accept/reject -> width-adaptation step of every chain."""
        self._check(self._lib.me_step(self._handle, int(n_sweeps)))
        if self.n_chains == 1:
            accepted, _ = self.accept_stats()
            took = accepted > self._last_accepted
            self._last_accepted = accepted
            return took if n_sweeps == 1 else None
        return None

    def step_injected(self, normals, uniforms, kind=_capi.STEP_ALL):
        """Test hook (float64 engines): step with caller-supplied draws instead of the Philox stream
        (``me_step_injected``): ``normals[sweep, chain, D]`` and ``uniforms[sweep, chain]`` for the Gaussian kinds,
        ``normals[sweep, chain, nc]`` and ``uniforms[sweep, chain, nc + 2]`` for the magnitude-phase pair.  On a ladder
        engine: step_all with the identity proposal shape only."""
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        nc = self.num_complex_params
        magphase = kind == _capi.STEP_COMPLEX_MAGNITUDE_PHASE
        nz = nc if magphase else self.num_real_params + 2 * nc
        want_u = normals.shape[:2] + ((nc + 2,) if magphase else ())
        if normals.ndim != 3 or normals.shape[1:] != (self.n_chains, nz) or uniforms.shape != want_u:
            raise ValueError("injected streams have the wrong shape for this step kind")
        self._check(self._lib.me_step_injected(self._handle, int(kind), normals.shape[0], _as_double_ptr(normals),
                                               _as_double_ptr(uniforms)))

    def _step_kind(self, kind, n_sweeps):
        before = self.accept_stats()[0] if self.n_chains == 1 else 0
        self._check(self._lib.me_step_kind(self._handle, int(kind), int(n_sweeps)))
        if self.n_chains == 1 and n_sweeps == 1 and kind != _capi.STEP_COMPLEX_MAGNITUDE_PHASE:
            accepted = self.accept_stats()[0]
            self._last_accepted = accepted
            return accepted > before
        return None                                   # the magnitude-phase pair returns None (:175-176)

    def step_real_group(self, n_sweeps=1):
        """metropolis_engine.py:225-239: only the real parameters move, only the real width adapts.  On pure-real
        engines this IS step_all (:56)."""
        return self._step_kind(_capi.STEP_REAL_GROUP, n_sweeps)

    def step_complex_group(self, n_sweeps=1):
        """metropolis_engine.py:209-223, or the magnitude-phase pair (:168-207) when the engine was built with
        ``complex_sample_method="magnitude-phase"``."""
        if self.complex_sample_method == "magnitude-phase":
            return self._step_kind(_capi.STEP_COMPLEX_MAGNITUDE_PHASE, n_sweeps)
        return self._step_kind(_capi.STEP_COMPLEX_GROUP, n_sweeps)

    def measure(self):
        """Update running means, covariances (once measure_step_counter > 50) and observables (:342-427)."""
        self._check(self._lib.me_measure(self._handle))

    def cycle(self, n_sweeps=1):
        """``n_sweeps`` x ``step_all()`` followed by ``measure()`` -- one iteration of the reference's driver loop
        (README.md:41-44) -- as ONE kernel launch where the engine has a fused kernel (``me_cycle``); same results as
        ``step_all(n_sweeps); measure()``."""
        self._check(self._lib.me_cycle(self._handle, int(n_sweeps)))

    def fused_cycles(self):
        """How many :meth:`cycle` calls ran as one launch (the others fell back to a step and a measure launch)."""
        count = ctypes.c_uint64()
        self._check(self._lib.me_cycle_stats(self._handle, ctypes.byref(count)))
        return count.value

    measure_real_system = measure                                                        # :57
    measure_complex_system = measure                                                     # :47

    # ------------------------------------------------------------------ setters (:136-149)
    def set_reject_condition(self, reject_fct):
        """metropolis_engine.py:142-146 (in the reference the only working way to install a constraint, quirk Q6).
        ``reject_fct`` is a :class:`~metropolisengine_amd.energy.RejectSpec`, ``None`` (no constraint) or -- on an engine whose
        energy is a Python callable -- a Python predicate ``(real_params, complex_params) -> bool``: energy and predicate are
        traced into one new plugin and the engine is re-bound to it."""
        if reject_fct is not None and not isinstance(reject_fct, RejectSpec):
            from .pyenergy import PythonEnergy, PythonReject
            if not callable(reject_fct):
                raise TypeError("reject_condition must be a RejectSpec, a callable or None")
            if not isinstance(self._energy_spec, PythonEnergy):
                raise TypeError("a Python reject_condition needs a Python energy (both are traced into one device plugin); "
                                "with a built-in energy use a RejectSpec such as AbsReal0AtLeast")
            self._bind_energy(PythonEnergy(self._energy_spec.energy, reject=reject_fct))
            reject_fct = PythonReject()
        kind = reject_fct.kind if reject_fct is not None else _capi.REJECT_NONE
        bound = reject_fct.bound if reject_fct is not None else 0.0
        self._check(self._lib.me_set_reject_condition(self._handle, int(kind), float(bound)))
        self._reject_spec = reject_fct

    def _bind_energy(self, spec):
        nr, nc = self.num_real_params, self.num_complex_params
        name = None
        if hasattr(spec, "ensure_loaded"):
            spec.ensure_loaded(nr, nc)
            name = spec.name.encode()
        coeffs = np.ascontiguousarray(spec.coefficients(nr, nc), dtype=np.float64)
        self._check(self._lib.me_set_energy(self._handle, int(spec.kind), _as_double_ptr(coeffs), int(coeffs.size), name))
        self._energy_spec = spec
        self._user_name = name
        self.energy_term_names = list(spec.term_names)

    def set_energy_function(self, energy_function):
        """metropolis_engine.py:134-138: replace the energy -- the reference's term dictionary, a single callable, or an
        :class:`~metropolisengine_amd.energy.EnergySpec` -- on the same parameter space.  The term names are collected anew
        and, unlike the reference (which leaves ``self.energy`` stale until ``initialize_energy_dict`` is called), every
        term is re-evaluated at the current state.  State, widths, running statistics and counters stay."""
        if not isinstance(energy_function, EnergySpec):
            if not (callable(energy_function) or isinstance(energy_function, dict)):
                raise TypeError("energy_function must be an EnergySpec, a callable or a dictionary of term callables")
            from .pyenergy import PythonEnergy
            keep = getattr(self._energy_spec, "reject", None) if isinstance(self._reject_spec, RejectSpec) and \
                self._reject_spec.kind == _capi.REJECT_USER else None
            energy_function = PythonEnergy(energy_function, reject=keep)
        self._bind_energy(energy_function)

    def initialize_energy_dict(self):
        """Re-evaluate every term of the energy ledger at the current state (metropolis_engine.py:152-155)."""
        self._check(self._lib.me_recompute_energy(self._handle))

    def set_initial_sampling_width(self, sampling_width):
        self.group_sampling_width = sampling_width                                       # :148-149 (unused there too)

    # ------------------------------------------------------------------ raw field access
    def _get(self, field, chain_begin=0, n_chains=None):
        n = self.n_chains - chain_begin if n_chains is None else n_chains
        comps = ctypes.c_int32()
        self._check(self._lib.me_field_components(self._handle, field, ctypes.byref(comps)))
        out = np.empty((n, comps.value), dtype=np.float64)
        self._check(self._lib.me_get(self._handle, field, chain_begin, n, _as_double_ptr(out)))
        return out

    def _set(self, field, values, chain_begin=0):
        values = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self._lib.me_set(self._handle, field, chain_begin, values.shape[0], _as_double_ptr(values)))

    def _squeeze(self, arr):
        return arr[0] if self.n_chains == 1 else arr

    # ------------------------------------------------------------------ the reference's attributes
    @property
    def real_params(self):
        return self._squeeze(self._get(_capi.FIELD_PARAMS)[:, :self.num_real_params])

    @property
    def complex_params(self):
        nr, nc = self.num_real_params, self.num_complex_params
        x = self._get(_capi.FIELD_PARAMS)
        return self._squeeze(x[:, nr:nr + nc] + 1j * x[:, nr + nc:])

    @property
    def real_mean(self):
        return self._squeeze(self._get(_capi.FIELD_MEAN)[:, :self.num_real_params])

    @property
    def complex_mean(self):
        nr, nc = self.num_real_params, self.num_complex_params
        x = self._get(_capi.FIELD_MEAN)
        return self._squeeze(x[:, nr:nr + nc] + 1j * x[:, nr + nc:])

    @property
    def covariance_matrix_real(self):
        if not self.num_real_params:
            return None
        return self._squeeze(unpack_real_block(self._get(_capi.FIELD_COV), self.num_real_params))

    @property
    def covariance_matrix_complex(self):
        if not self.num_complex_params:
            return None
        return self._squeeze(unpack_complex_block(self._get(_capi.FIELD_COV), self.num_real_params,
                                                  self.num_complex_params))

    @property
    def observables(self):
        nr, nc = self.num_real_params, self.num_complex_params
        x = self._get(_capi.FIELD_PARAMS)
        z = x[:, nr:nr + nc] + 1j * x[:, nr + nc:]
        return self._squeeze(np.concatenate((np.abs(x[:, :nr]), np.abs(z), x[:, :nr] ** 2), axis=1))   # :458-463

    @property
    def observables_mean(self):
        return self._squeeze(self._get(_capi.FIELD_OBS_MEAN))

    def _width(self, row):
        w = self._get(_capi.FIELD_WIDTH)       # [n, 1], or [n, 3] = (sampling_width, real, complex) for mixed engines
        w = w[:, row if w.shape[1] == 3 else 0]
        return float(w[0]) if self.n_chains == 1 else w

    @property
    def sampling_width(self):
        return self._width(0)

    @property
    def real_group_sampling_width(self):
        # pure-complex engines never touch the real width (:449-456)
        return self._width(1) if self.num_real_params else self._initial_widths[0]

    @property
    def complex_group_sampling_width(self):
        return self._width(2) if self.num_complex_params else self._initial_widths[1]

    @property
    def energy_total(self):
        if self.reference_energy_ledgers:                  # the reference's separate attribute (quirk Q5)
            e = self._get(_capi.FIELD_ENERGY_TOTAL)[:, 0]
        else:
            e = self._get(_capi.FIELD_ENERGY).sum(axis=1)     # sum of the ledger's terms (:158-162)
        return float(e[0]) if self.n_chains == 1 else e

    @property
    def energy(self):
        """The energy ledger, ``{term name: value}`` (``self.energy``, :152-155); one entry ``"total"`` unless the
        energy is a term dictionary."""
        rows = self._get(_capi.FIELD_ENERGY)
        return {name: (float(rows[0, t]) if self.n_chains == 1 else rows[:, t])
                for t, name in enumerate(self.energy_term_names)}

    def _counters(self):
        step, meas = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.me_counters(self._handle, ctypes.byref(step), ctypes.byref(meas)))
        return step.value, meas.value

    @property
    def measure_step_counter(self):
        return self._counters()[1]

    @property
    def step_counter(self):
        # starts at 1 and counts width updates (:72, :450); every GPU step updates the width
        return self._counters()[0] + 1

    # ------------------------------------------------------------------ many-chain extras
    def sync(self):
        self._check(self._lib.me_sync(self._handle))

    def accept_stats(self):
        """(accepted, proposed) chain-steps so far (ballot-reduced on the device)."""
        acc, prop = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.me_accept_stats(self._handle, ctypes.byref(acc), ctypes.byref(prop)))
        return acc.value, prop.value

    def acceptance_rate(self):
        acc, prop = self.accept_stats()
        return acc / prop if prop else float("nan")

    def pooled_moments(self):
        """Local ensemble sums (fp64), layout of ``me_pooled_moments`` in include/metropolis_engine.h."""
        size = ctypes.c_int64()
        self._check(self._lib.me_pooled_moments_size(self._handle, ctypes.byref(size)))
        out = np.empty(size.value, dtype=np.float64)
        self._check(self._lib.me_pooled_moments(self._handle, _as_double_ptr(out), size.value))
        return out

    def pooled_moments_geometry(self):
        """(matrix_core, tile_chains, partial_rows) of the first stage :meth:`pooled_moments` launches: whether it is the
        kernel set's Gram kernel, the chains it stages per tile, and its rows of partial sums."""
        core, tile, rows = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.me_pooled_moments_geometry(self._handle, ctypes.byref(core), ctypes.byref(tile), ctypes.byref(rows)))
        return bool(core.value), tile.value, rows.value

    def pooled_moments_begin(self):
        """Enqueue the pooled-moment reduction of the CURRENT state and its copy to the host without waiting; work
        enqueued afterwards overlaps it.  Collect with :meth:`pooled_moments_end`."""
        self._check(self._lib.me_pooled_moments_begin(self._handle))

    def pooled_moments_end(self):
        size = ctypes.c_int64()
        self._check(self._lib.me_pooled_moments_size(self._handle, ctypes.byref(size)))
        out = np.empty(size.value, dtype=np.float64)
        self._check(self._lib.me_pooled_moments_end(self._handle, _as_double_ptr(out), size.value))
        return out

    # ------------------------------------------------------------------ temperature ladders and replica exchange
    @property
    def temperatures(self):
        """The ladder ``T_0 < ... < T_{K-1}`` as a ``(K,)`` array, or ``None`` (every chain at ``temp``)."""
        k = ctypes.c_int32()
        self._check(self._lib.me_temperature_ladder(self._handle, None, 0, ctypes.byref(k)))
        if k.value == 0:
            return None
        out = np.empty(k.value, dtype=np.float64)
        self._check(self._lib.me_temperature_ladder(self._handle, _as_double_ptr(out), k.value, ctypes.byref(k)))
        return out

    def set_temperatures(self, temperatures):
        """Install a ladder (``me_set_temperature_ladder``): the chains become ``K`` rungs of ``n_chains / K`` consecutive
        chains, rung ``k`` stepping at ``temperatures[k]``; the swap round and counters start over.  ``None`` returns the
        engine to its scalar ``temp``.  ``NotImplementedError`` on engines that cannot carry a ladder (runtime dimensions,
        the dense 64-parameter matrix-core form, ``reference_energy_ledgers=True``)."""
        if temperatures is None:
            self._check(self._lib.me_set_temperature_ladder(self._handle, None, 0))
            return
        if self.temp != 0:
            raise ValueError("this engine has a scalar temp; a ladder engine is created with temp=0")
        temps = np.ascontiguousarray(validate_ladder(temperatures, self.n_chains))
        self._check(self._lib.me_set_temperature_ladder(self._handle, _as_double_ptr(temps), temps.size))

    def replica_exchange(self, n_rounds=1):
        """Enqueue ``n_rounds`` replica-exchange rounds (asynchronous, like :meth:`step_all`): round ``r`` offers slot ``j``
        of rung ``k`` and slot ``j`` of rung ``k+1`` a swap of their configurations for every ``k = r (mod 2)``."""
        self._check(self._lib.me_replica_exchange(self._handle, int(n_rounds)))

    def swap_stats(self):
        """``(round, attempted, accepted)``: the next round's number and the swaps per adjacent pair of rungs, ``(K-1,)``."""
        temps = self.temperatures
        if temps is None:
            raise ValueError("this engine has no temperature ladder")
        n_pairs = temps.size - 1
        rnd = ctypes.c_uint64()
        att = (ctypes.c_uint64 * max(n_pairs, 1))()
        acc = (ctypes.c_uint64 * max(n_pairs, 1))()
        self._check(self._lib.me_replica_stats(self._handle, ctypes.byref(rnd), att, acc, n_pairs))
        return (rnd.value, np.array(att[:n_pairs], dtype=np.int64), np.array(acc[:n_pairs], dtype=np.int64))

    def swap_acceptance(self):
        """Accepted / attempted swaps per adjacent pair of rungs, ``(K-1,)`` (NaN before the pair's first attempt)."""
        _, att, acc = self.swap_stats()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(att > 0, acc / np.maximum(att, 1), np.nan)

    def chain_temperatures(self):
        """The temperature each local chain steps at, ``(n_chains,)``."""
        temps = self.temperatures
        if temps is None:
            return np.full(self.n_chains, float(self.temp))
        return np.repeat(temps, self.n_chains // temps.size)

    def pooled_moments_by_rung(self):
        """:meth:`pooled_moments` of every rung, ``(K, moments_size)`` (``me_pooled_moments_range``); the two trailing
        counters of a rung are 0 (acceptance is counted per launch wavefront, not per chain).  Without a ladder: one row,
        the whole engine."""
        temps = self.temperatures
        if temps is None:
            return self.pooled_moments()[None, :]
        size = ctypes.c_int64()
        self._check(self._lib.me_pooled_moments_size(self._handle, ctypes.byref(size)))
        m = self.n_chains // temps.size
        out = np.empty((temps.size, size.value), dtype=np.float64)
        for k in range(temps.size):
            self._check(self._lib.me_pooled_moments_range(self._handle, k * m, m, _as_double_ptr(out[k]), size.value))
        return out

    # ------------------------------------------------------------------ energy samples, MBAR free energies, reweighting
    def record_energies(self, capacity):
        """Allocate a device store for ``capacity`` records of every chain's energy (``me_energy_samples_enable``; float64,
        ``capacity * n_chains * 8`` bytes) and forget the records so far; ``0`` frees it.  ``ValueError`` for a negative
        capacity, ``NotImplementedError`` with ``reference_energy_ledgers=True``.

        The samples are NOT part of :meth:`state_dict` (they can be hundreds of megabytes): a run is resumed with
        :meth:`energy_samples` / :meth:`set_energy_samples`.  :meth:`set_temperatures` empties the store, because a sample's
        temperature is the rung of its slot."""
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        self._check(self._lib.me_energy_samples_enable(self._handle, capacity))

    def record_energy(self):
        """Append one record: the energy of every chain now, the ledger rows summed in row order in the device dtype
        (``me_energy_samples_record``; one kernel, asynchronous like :meth:`step_all`).  Raises when the store was never
        enabled or is full."""
        self._check(self._lib.me_energy_samples_record(self._handle))

    def _energy_records(self):
        rows, cap = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.me_energy_samples_count(self._handle, ctypes.byref(rows), ctypes.byref(cap)))
        return rows.value, cap.value

    @property
    def n_energy_records(self):
        return self._energy_records()[0]

    def energy_samples(self):
        """The recorded energies, ``(records, n_chains)`` float64; column ``c`` is slot ``c``, i.e. rung ``c // M``."""
        rows = self.n_energy_records
        out = np.empty((rows, self.n_chains), dtype=np.float64)
        if rows:
            self._check(self._lib.me_energy_samples_get(self._handle, 0, rows, _as_double_ptr(out)))
        return out

    def set_energy_samples(self, samples):
        """Replace the records by ``samples`` (``(records, n_chains)``, at most the capacity of :meth:`record_energies`)."""
        a = np.ascontiguousarray(samples, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.n_chains:
            raise ValueError("samples must be (records, n_chains = %d)" % self.n_chains)
        self._check(self._lib.me_energy_samples_set(self._handle, a.shape[0], _as_double_ptr(a)))

    def ladder_free_energies(self, tol=1e-10, max_iter=10000, method="self-consistent"):
        """MBAR over the recorded energies of a ladder engine (``me_mbar_solve``, on the device): ``{"f", "ln_z",
        "iterations", "residual", "converged", "n_samples"}`` with ``f[k] = -ln Z(T_k) / Z(T_0)``, ``ln_z = -f``, the
        iterations taken, the last largest change of an ``f[k]``, whether it met ``tol``, and the finite samples of every
        rung (non-finite energies are skipped).  Bitwise reproducible.  ``ValueError`` unless ``tol > 0`` and ``max_iter >=
        1``; raises without a ladder, without records, or when a rung has no finite sample.  ``method="newton"`` takes
        Newton steps after two self-consistent ones (``me_mbar_solve_newton``: quadratic convergence; every pass over the
        samples is an iteration) and adds ``gradient`` (``max_k |S_k / N_k - 1|`` at the last pass), ``newton_steps`` and
        ``fallback_steps``; any other ``method`` is a ``ValueError``."""
        from . import statistics
        method = statistics.validate_mbar_method(method)
        tol, max_iter = statistics.validate_mbar_solve(tol, max_iter)
        k = ctypes.c_int32()
        self._check(self._lib.me_temperature_ladder(self._handle, None, 0, ctypes.byref(k)))
        if method == "newton":
            return statistics._solve_newton(self._lib.me_mbar_solve_newton, (self._handle,), max(k.value, 1), tol, max_iter)
        return statistics._solve(self._lib.me_mbar_solve, (self._handle,), max(k.value, 1), tol, max_iter)

    def _ladder_f(self, f, finite):
        """``f`` checked against the ladder, if there is one (``statistics.validate_mbar_f``)."""
        from . import statistics
        ladder = self.temperatures
        return statistics.validate_mbar_f(f, None if ladder is None else ladder.size, finite)

    def reweight(self, temps, f=None):
        """The ladder's samples reweighted to each temperature of ``temps`` (``me_mbar_reweight``): ``{"temps", "ln_z",
        "energy_mean", "energy_var", "heat_capacity", "neff_fraction"}`` -- ``ln Z(T) / Z(T_0)``, the mean and variance of
        the energy at ``T``, ``energy_var / T^2`` and the effective fraction of the samples behind the estimate.  ``f``: the
        free energies of :meth:`ladder_free_energies` (solved with the defaults when ``None``).  ``ValueError`` for empty,
        non-finite or non-positive ``temps``."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)      # (whether it is finite is the library's to say)
        return statistics._reweight(self._lib.me_mbar_reweight, (self._handle,), f, temps)

    def ladder_free_energy_uncertainties(self, f, targets=None, inefficiency=1.0):
        """Asymptotic standard errors of the ladder's MBAR free energies ``f`` (of :meth:`ladder_free_energies`) and, with
        ``targets``, of the reweighted ``ln_z`` and mean energy at those temperatures (``me_mbar_gram``: one further pass
        over the recorded samples; see :func:`metropolisengine_amd.statistics.mbar_uncertainties` for the dictionary).  The
        formula assumes independent samples: pass the statistical inefficiency of the energy series
        (:func:`metropolisengine_amd.statistics.statistical_inefficiency`) as ``inefficiency`` (finite, ``>= 1``) and every
        variance is multiplied by it.  ``inefficiency="recorded"`` takes it from the records themselves: the largest energy
        ``g`` over the rungs of :meth:`recorded_inefficiency` (deliberately conservative: one scalar has to serve every rung).
        ``ValueError`` for invalid ``targets`` or ``inefficiency``; raises like :meth:`ladder_free_energies` without a ladder or
        without records."""
        from . import statistics
        if isinstance(inefficiency, str):
            inefficiency = self._recorded_g(inefficiency, [()])[0]
        g = statistics.validate_mbar_inefficiency(inefficiency)
        if targets is not None:
            targets = statistics.validate_mbar_temps(targets, "targets")
        f = self._ladder_f(f, finite=True)
        k = max(f.size, 1)      # (the ladder's rungs; without a ladder the library refuses before it writes)

        def energy_shift():     # of the energy columns, from the device: the samples stay there
            shift = ctypes.c_double(0.0)
            self._check(self._lib.me_mbar_energy_shift(self._handle, ctypes.byref(shift)))
            return shift.value
        return statistics._uncertainties(self._lib.me_mbar_gram, (self._handle,), k, f, targets, g, energy_shift)

    # ------------------------------------------------------------------ recorded observables and their reweighting
    def observable_names(self):
        """The catalogue of a chain's recordable quantities, in the order of the C ABI (``me_observable_samples_enable``):
        the state rows ``real_i``, ``re_i``, ``im_i``; the observables ``abs_real_i``, ``abs_complex_i``, ``real_i_sq`` (the
        order of :attr:`observables_mean`); the ledger rows ``energy_<term name>``."""
        from .statistics import observable_catalogue
        return observable_catalogue(self.num_real_params, self.num_complex_params, self.energy_term_names)

    def record_observables(self, which):
        """Record per-chain observables next to every energy record from now on (``me_observable_samples_enable``; call it
        after :meth:`record_energies`, whose capacity it takes: float64, ``capacity * len(which) * n_chains * 8`` bytes on the
        device).  ``which``: up to 16 names of :meth:`observable_names` or indices into it (duplicates allowed); ``None`` or
        an empty sequence frees the store.  The records of BOTH stores so far are forgotten, so record ``r`` of
        :meth:`energy_samples` and of :meth:`observable_samples` is always the same moment; :meth:`record_energies` frees the
        observable store and :meth:`set_temperatures` empties both.  ``ValueError`` for unknown names, indices outside the
        catalogue, more than 16 entries or no energy store; ``NotImplementedError`` with ``reference_energy_ledgers=True``.

        Like the energy samples, the observable samples are NOT part of :meth:`state_dict`: a run is resumed with
        :meth:`set_energy_samples` followed by :meth:`set_observable_samples`."""
        from .statistics import validate_observable_selection
        if which is None or len(which) == 0:
            self._check(self._lib.me_observable_samples_enable(self._handle, None, 0))
            return
        idx = validate_observable_selection(which, self.observable_names())
        status = self._lib.me_observable_samples_enable(self._handle, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), idx.size)
        if status == _capi.ME_ERR_STATE:         # no energy store
            raise ValueError(_capi.last_error(self._handle))
        self._check(status)

    def _recorded_observable_indices(self):
        n = ctypes.c_int32()
        idx = np.zeros(16, dtype=np.int32)
        self._check(self._lib.me_observable_samples_info(self._handle, ctypes.byref(n), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return idx[:n.value]

    @property
    def recorded_observables(self):
        """The names of the recorded columns, in column order (empty without an observable store)."""
        names = self.observable_names()
        return tuple(names[i] for i in self._recorded_observable_indices())

    def observable_samples(self):
        """The recorded observables, ``(records, Q, n_chains)`` float64, record ``r`` taken with energy record ``r``."""
        q = self._recorded_observable_indices().size
        if q == 0:
            raise ValueError("no observable store: call record_observables first")
        rows = self.n_energy_records
        out = np.empty((rows, q, self.n_chains), dtype=np.float64)
        if rows:
            self._check(self._lib.me_observable_samples_get(self._handle, 0, rows, _as_double_ptr(out)))
        return out

    def set_observable_samples(self, samples):
        """Replace the observable records by ``samples``, ``(records, Q, n_chains)`` with ``records`` equal to the current
        number of energy records (call :meth:`set_energy_samples` first)."""
        q = self._recorded_observable_indices().size
        if q == 0:
            raise ValueError("no observable store: call record_observables first")
        a = np.ascontiguousarray(samples, dtype=np.float64)
        if a.ndim != 3 or a.shape[1:] != (q, self.n_chains):
            raise ValueError("samples must be (records, Q = %d, n_chains = %d)" % (q, self.n_chains))
        self._check(self._lib.me_observable_samples_set(self._handle, a.shape[0], _as_double_ptr(a)))

    def reweight_observables(self, temps, f=None):
        """The recorded observables reweighted to each temperature of ``temps`` (``me_mbar_reweight_observables``, on the
        device): ``{"temps", "names", "mean", "var", "cov_energy", "dmean_dT", "neff_fraction"}`` -- the MBAR estimates of
        ``<A_q>``, of its variance and of its covariance with the energy at ``T``, all ``(T, Q)``, ``dmean_dT = cov_energy /
        T^2`` (the temperature derivative of the mean) and the effective fraction of the samples, ``(T,)``.  ``f``: the free
        energies of :meth:`ladder_free_energies` (solved with the defaults when ``None``).  Bitwise reproducible, and column
        ``q`` at temperature ``t`` does not depend on what else is asked for.  ``ValueError`` for empty, non-finite or
        non-positive ``temps``; raises without a ladder, without records or without an observable store."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        names = self.recorded_observables
        if not names:
            raise ValueError("no observable store: call record_observables first")
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        return statistics._reweight_observables(self._lib.me_mbar_reweight_observables, (self._handle,), f, temps, names)

    def reweight_perturbed(self, temps, couplings, f=None):
        """The ladder's samples reweighted to states that differ by more than their temperature
        (``me_mbar_reweight_perturbed``, on the device): target ``p`` has the temperature ``temps[p]`` (a scalar serves every
        target) and the energy ``H = E + sum_q couplings[p, q] A_q`` over the recorded columns ``A_q`` -- a field conjugate to
        an order parameter (``{"real_0": -h}``), a changed stiffness (``{"real_0_sq": lam}``), a changed coefficient of one
        term of an energy dictionary (``{"energy_<term>": c_new / c - 1}``).  ``couplings``: ``(P, Q)`` in the order of
        :attr:`recorded_observables`, or a dictionary from recorded names or column indices to scalars or ``(P,)``; columns
        it does not name are 0.  ``f``: the free energies of :meth:`ladder_free_energies` (solved with the defaults when
        ``None``).  Returns ``{"temps", "couplings" (P, Q), "names", "ln_z", "hamiltonian_mean", "hamiltonian_var",
        "heat_capacity", "perturbation_mean", "mean", "var", "cov_hamiltonian", "dmean_dT", "neff_fraction"}`` (see
        :func:`metropolisengine_amd.statistics.mbar_reweight_perturbed`).  Bitwise reproducible; a target does not depend on
        what else is asked for, and a column whose coupling is exactly 0 never enters ``H``.  ``ValueError`` for invalid
        ``temps`` or ``couplings`` (shape, unknown name, a column named twice, non-finite); raises without a ladder, without
        records or without an observable store."""
        from . import statistics
        temps = statistics.broadcast_mbar_targets(temps, couplings)
        names = self.recorded_observables
        if not names:
            raise ValueError("no observable store: call record_observables first")
        lam = statistics.validate_mbar_couplings(couplings, temps.size, names)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        return statistics._reweight_perturbed(self._lib.me_mbar_reweight_perturbed, (self._handle,), f, temps, lam, names)

    def free_energy_profile(self, which, edges, temps, f=None):
        """The reweighted histogram of one recorded quantity and the free-energy profile ``F(A; T) = -T ln p(A; T)`` along it at
        each temperature of ``temps`` (``me_mbar_histogram``, on the device: the samples stay there).  ``which``: a name of
        :attr:`recorded_observables`, an index into the recorded columns, or ``"energy"`` (the recorded energies themselves,
        which need no observable store).  ``edges``: 2 to 257 finite, strictly increasing bin edges of any spacing.  ``f``: the
        free energies of :meth:`ladder_free_energies` (solved with the defaults when ``None``).

        Every sample with a finite energy falls into exactly one slot: bin ``b`` when ``edges[b] <= A < edges[b + 1]``
        (half-open everywhere), *below*, *above* (``A >= edges[-1]``: a value equal to the LAST edge is above, unlike
        ``np.histogram``, which closes its last bin) or *not a number*.  Returns ``{"temps", "name", "edges", "centers",
        "widths", "mass", "below", "above", "not_a_number", "density", "free_energy", "counts", "counts_outside",
        "neff_fraction"}``, see :func:`metropolisengine_amd.statistics.mbar_free_energy_profile`.  Bitwise reproducible, and
        a temperature's row does not depend on which others are asked for.  ``ValueError`` for bad edges, an unknown name, an
        index outside the recorded columns and empty, non-finite or non-positive ``temps``; raises without a ladder or
        without records."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        edges = statistics.validate_histogram_edges(edges)
        column, name = self._profile_column(which)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        out = statistics._free_energy_profile(self._lib.me_mbar_histogram, (self._handle,), f, temps, (column,), edges)
        out["name"] = name
        return out

    def free_energy_profile_uncertainties(self, which, edges, temps, f=None, inefficiency=1.0):
        """:meth:`free_energy_profile` with the asymptotic standard errors of the masses and of the profile
        (``me_mbar_histogram_gram``, on the device: ``K + 1`` weighted histograms per temperature and the ladder block of the
        Gram matrix; the samples stay there).  Arguments as there.  Returns every key of :meth:`free_energy_profile`, bit for
        bit, and ``{"d_mass", "d_below", "d_above", "d_not_a_number", "d_free_energy", "log_mass_cov",
        "d_free_energy_from_lowest", "lowest", "n_samples"}``, see
        :func:`metropolisengine_amd.statistics.mbar_free_energy_profile_uncertainties`: the error of a barrier height ``F_b -
        F_b'`` at temperature ``t`` is ``T sqrt(C[b, b] + C[b', b'] - 2 C[b, b'])`` with ``C = log_mass_cov[t]``.
        ``inefficiency``: the statistical inefficiency of the recorded series, a finite scalar ``>= 1`` that multiplies every
        variance, or ``"recorded"``: the largest ``g`` of :meth:`recorded_inefficiency` over the rungs and over the energy (the
        weights depend on it) and ``which`` (the slots do); deliberately conservative.  ``ValueError`` as
        :meth:`free_energy_profile` and for an invalid ``inefficiency``; raises without a ladder or without records."""
        from . import statistics
        if isinstance(inefficiency, str):
            column = self._profile_column(which)[0]
            inefficiency = self._recorded_g(inefficiency, [() if column < 0 else (column,)])[0]
        g = statistics.validate_profile_inefficiency(inefficiency)
        temps = statistics.validate_mbar_temps(temps)
        edges = statistics.validate_histogram_edges(edges)
        column, name = self._profile_column(which)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        k = max(f.size, 1)      # (the ladder's rungs; without a ladder the library refuses before it writes)
        out = statistics._free_energy_profile_uncertainties(self._lib.me_mbar_histogram_gram, (self._handle,), k, f, temps, (column,),
                                                            edges, g)
        out["name"] = name
        return out

    def free_energy_surface(self, which_x, edges_x, which_y, edges_y, temps, f=None):
        """The joint reweighted histogram of two recorded quantities and the free-energy surface ``F(A, B; T) = -T ln p(A, B;
        T)`` over them at each temperature of ``temps`` (``me_mbar_histogram_joint``, on the device: the samples stay there).
        ``which_x``, ``which_y``: as :meth:`free_energy_profile`'s ``which`` -- a name of :attr:`recorded_observables`, an
        index into the recorded columns, or ``"energy"``; the same quantity may be given twice.  Each axis has edges of its
        own as there, and the ``(Bx + 3)(By + 3)`` cells may not exceed 1296 (33 x 33 bins).  ``f``: the free energies of
        :meth:`ladder_free_energies` (solved with the defaults when ``None``).

        Every sample with a finite energy falls into exactly one cell: per axis a bin, *below*, *above* or *not a number* by
        the rule of :meth:`free_energy_profile`.  Returns ``{"temps", "names", "edges_x", "edges_y", "centers_x",
        "centers_y", "widths_x", "widths_y", "mass", "density", "free_energy", "mass_slots", "outside", "counts",
        "counts_slots", "neff_fraction"}``, see :func:`metropolisengine_amd.statistics.mbar_free_energy_surface`; ``names`` is
        the pair of the axes' names.  Bitwise reproducible, and a temperature's table does not depend on which others are asked
        for.  ``ValueError`` for bad edges, too many cells, an unknown name, an index outside the recorded columns and empty,
        non-finite or non-positive ``temps``; raises without a ladder or without records."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        edges_x, edges_y = statistics.validate_histogram2d_edges(edges_x, edges_y)
        (column_x, name_x), (column_y, name_y) = self._profile_column(which_x), self._profile_column(which_y)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        out = statistics._free_energy_surface(self._lib.me_mbar_histogram_joint, (self._handle,), f, temps, (column_x,), edges_x,
                                              (column_y,), edges_y)
        out["names"] = (name_x, name_y)
        return out

    def free_energy_surface_uncertainties(self, which_x, edges_x, which_y, edges_y, temps, f=None, inefficiency=1.0,
                                          covariance=True):
        """:meth:`free_energy_surface` with the asymptotic standard errors of the masses and of the surface
        (``me_mbar_histogram_joint_gram``, on the device: ``K + 1`` weighted joint histograms per temperature and the ladder
        block of the Gram matrix; the samples stay there).  Arguments as there.  Returns every key of
        :meth:`free_energy_surface`, bit for bit, and ``{"d_mass", "d_mass_slots", "d_outside", "d_free_energy", "lowest",
        "d_free_energy_from_lowest", "n_samples"}`` and, with ``covariance=True``, ``"log_mass_cov"`` ``(T, Bx By, Bx By)``, see
        :func:`metropolisengine_amd.statistics.mbar_free_energy_surface_uncertainties`: the error of a saddle height ``F_c -
        F_c'`` at temperature ``t`` is ``T sqrt(C[c, c] + C[c', c'] - 2 C[c, c'])`` with ``C = log_mass_cov[t]`` and the cell
        index ``bx * By + by``.  ``covariance=False`` leaves that matrix out (9.5 MB per temperature at 33 x 33 bins).
        ``inefficiency``: the statistical inefficiency of the recorded series, a finite scalar ``>= 1`` that multiplies every
        variance, or ``"recorded"``: the largest ``g`` of :meth:`recorded_inefficiency` over the rungs and over the energy (the
        weights depend on it), ``which_x`` and ``which_y`` (the cells do); deliberately conservative.  ``ValueError`` as
        :meth:`free_energy_surface` and for an invalid ``inefficiency`` or ``covariance``; raises without a ladder or without
        records."""
        from . import statistics
        covariance = statistics.validate_surface_covariance(covariance)
        if isinstance(inefficiency, str):
            columns = tuple(sorted({c for c in (self._profile_column(which_x)[0], self._profile_column(which_y)[0]) if c >= 0}))
            inefficiency = self._recorded_g(inefficiency, [columns])[0]
        g = statistics.validate_profile_inefficiency(inefficiency)
        temps = statistics.validate_mbar_temps(temps)
        edges_x, edges_y = statistics.validate_histogram2d_edges(edges_x, edges_y)
        (column_x, name_x), (column_y, name_y) = self._profile_column(which_x), self._profile_column(which_y)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=False)
        k = max(f.size, 1)      # (the ladder's rungs; without a ladder the library refuses before it writes)
        out = statistics._free_energy_surface_uncertainties(self._lib.me_mbar_histogram_joint_gram, (self._handle,), k, f, temps,
                                                            (column_x,), edges_x, (column_y,), edges_y, g, covariance)
        out["names"] = (name_x, name_y)
        return out

    def _profile_column(self, which):
        """``(column of the C ABI, name)`` of the quantity a profile runs along: -1 for ``"energy"``."""
        if isinstance(which, str) and which == "energy":
            return -1, "energy"
        names = self.recorded_observables
        if not names:
            raise ValueError("no observable store: call record_observables first")
        if isinstance(which, str):
            if which not in names:
                raise ValueError("unknown recorded observable %r; this engine records %s" % (which, ", ".join(names)))
            column = names.index(which)
        elif isinstance(which, (int, np.integer)) and not isinstance(which, bool):
            if not 0 <= int(which) < len(names):
                raise ValueError("column %d outside the %d recorded columns" % (int(which), len(names)))
            column = int(which)
        else:
            raise ValueError("the quantity is named by str or int, got %r" % (which,))
        return column, names[column]

    def observable_uncertainties(self, temps, f=None, inefficiency=1.0):
        """Asymptotic standard errors of :meth:`reweight_observables`' means (``me_mbar_gram_observables``: one further pass
        over the recorded samples on the matrix cores): ``{"temps", "names", "mean", "d_mean", "mean_cov", "ln_z", "d_ln_z",
        "n_samples"}``, see :func:`metropolisengine_amd.statistics.mbar_observable_uncertainties`.  ``f``: the free energies of
        :meth:`ladder_free_energies` (solved with the defaults when ``None``).  ``inefficiency``: the statistical inefficiency
        of the recorded series, a scalar or one entry per recorded column (finite, ``>= 1``), or ``"recorded"``: per column the
        largest ``g`` of :meth:`recorded_inefficiency` over the rungs and over the energy (the weights depend on it) and the
        column itself; deliberately conservative.  ``ValueError`` for invalid ``temps`` or ``inefficiency`` and without an
        observable store; raises without a ladder or without records."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        names = self.recorded_observables
        if not names:
            raise ValueError("no observable store: call record_observables first")
        if isinstance(inefficiency, str):
            inefficiency = self._recorded_g(inefficiency, [(q,) for q in range(len(names))])
        g = statistics.validate_mbar_observable_inefficiency(inefficiency, len(names))
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=True)
        k = max(f.size, 1)      # (the ladder's rungs; without a ladder the library refuses before it writes)
        return statistics._observable_uncertainties(self._lib.me_mbar_gram_observables, (self._handle,), k, f, temps, names, g)

    def fluctuation_uncertainties(self, temps, f=None, inefficiency=1.0):
        """Asymptotic standard errors of the reweighted second moments (``me_mbar_gram_fluctuations``: one further pass over the
        recorded samples on the matrix cores): of :meth:`reweight`'s ``energy_mean``, ``energy_var`` and ``heat_capacity`` and,
        with an observable store, of :meth:`reweight_observables`' ``mean``, ``var``, ``cov_energy`` and ``dmean_dT`` -- each
        value with its error under ``"d_" + key``, and ``{"temps", "names", "n_samples"}``, see
        :func:`metropolisengine_amd.statistics.mbar_fluctuation_uncertainties`.  Without an observable store the energy keys are
        computed alone and the others are ``(T, 0)``.  ``f``: the free energies of :meth:`ladder_free_energies` (solved with the
        defaults when ``None``).  ``inefficiency``: the statistical inefficiency of the recorded series, a finite scalar ``>= 1``
        that multiplies every variance, or ``"recorded"``: the largest ``g`` of :meth:`recorded_inefficiency` over the rungs, the
        energy and every recorded column; deliberately conservative.  ``ValueError`` for invalid ``temps`` or ``inefficiency``;
        raises without a ladder or without records."""
        from . import statistics
        temps = statistics.validate_mbar_temps(temps)
        names = tuple(self.recorded_observables or ())
        if isinstance(inefficiency, str):
            inefficiency = self._recorded_g(inefficiency, [tuple(range(len(names)))])[0]
        g = statistics.validate_profile_inefficiency(inefficiency)
        if f is None:
            f = self.ladder_free_energies()["f"]
        f = self._ladder_f(f, finite=True)
        k = max(f.size, 1)      # (the ladder's rungs; without a ladder the library refuses before it writes)
        return statistics._fluctuation_uncertainties(self._lib.me_mbar_gram_fluctuations, (self._handle,), k, f, temps, names, g)

    # ------------------------------------------------------------------ statistical inefficiency of the recorded series
    def recorded_inefficiency(self, mintime=3, max_lag=None):
        """The statistical inefficiency ``g = 1 + 2 tau`` of the recorded series, per column and rung, pooled over the chains of
        the rung (``me_recorded_inefficiency``, on the device: the stores stay there).  The records are successive states of
        Metropolis chains and never independent; a slot keeps its rung whatever configuration a swap put there, so the records
        of slot ``c`` are a stationary series at ``T[c // M]``, the series MBAR's samples come from.  The estimator is the
        multiple-series one of Chodera et al., JCTC 3:26 (2007), see
        :func:`metropolisengine_amd.statistics.series_inefficiency` for the formulas, ``mintime`` and ``max_lag``.

        Returns ``{"names": ("energy", *recorded_observables), "g", "tau" (= (g - 1) / 2), "mean", "var", "stop_lag",
        "chains_used"}``, each ``(1 + Q, K)``, ``"acf"`` ``(1 + Q, K, max_lag + 1)`` and ``"n_records"``.  Works without a ladder
        too: ``K = 1`` and the rung is the whole engine.  A chain with a non-finite value in a column is left out of that column
        (``chains_used``); a (column, rung) without a chain or without variance has ``g`` NaN.  Bitwise reproducible.
        ``ValueError`` for a bad ``mintime`` or ``max_lag``; raises without an energy store or with fewer than 3 records."""
        from . import statistics
        rows = self.n_energy_records
        if rows >= 3:
            mintime, max_lag = statistics.validate_series_lags(rows, mintime, max_lag)
        else:                   # (the library refuses, and says why)
            mintime, max_lag = 0, 1
        names = ("energy",) + self.recorded_observables
        ladder = self.temperatures
        out = statistics._series_inefficiency(self._lib.me_recorded_inefficiency, (self._handle,), len(names),
                                              1 if ladder is None else ladder.size, rows, mintime, max_lag)
        out["names"] = names
        return out

    def _recorded_g(self, inefficiency, columns):
        """``inefficiency="recorded"`` of the uncertainty methods: for each entry of ``columns`` (a tuple of recorded columns)
        the largest ``g`` of :meth:`recorded_inefficiency` over the rungs, over the energy and over those columns."""
        if inefficiency != "recorded":
            raise ValueError("inefficiency must be a number or \"recorded\", not %r" % (inefficiency,))
        g = self.recorded_inefficiency()["g"]
        out = np.array([float(np.max(g[[0] + [1 + q for q in entry]])) for entry in columns])
        if not np.all(np.isfinite(out)):
            raise ValueError("inefficiency=\"recorded\": a recorded series it needs has no statistical inefficiency (no chain "
                             "with finite values only, or no variance); see recorded_inefficiency()")
        return out

    # ------------------------------------------------------------------ scalar temperature and population annealing
    def set_temp(self, temp):
        """Change the scalar temperature of the running engine (``me_set_temperature``); the next step uses it, so a schedule
        of ``set_temp`` + :meth:`step_all` is plain simulated annealing.  ``temp`` finite and ``>= 0`` (``ValueError``
        otherwise, and on a ladder engine, whose rungs carry the temperatures)."""
        temp = float(temp)
        if not (np.isfinite(temp) and temp >= 0):
            raise ValueError("temp must be finite and >= 0")
        if self.temperatures is not None:
            raise ValueError("this engine has a temperature ladder: set_temperatures changes it")
        self._check(self._lib.me_set_temperature(self._handle, temp))
        self.temp = temp
        self._population_used = True

    def resample(self, temp):
        """One population-annealing stage (``me_population_resample``, asynchronous): reweight every chain by
        ``exp(-(1/temp - 1/self.temp) E)``, record the stage's estimate of ``ln Z(temp) / Z(self.temp)``, resample the
        population systematically in proportion to the weights and continue at ``temp``.  A slot receives its ancestor's
        configuration (parameters, energy ledger) and family id; everything adapted or measured (widths, running means,
        covariances, factors, traces, counters) stays with the slot.  ``ValueError`` for a ``temp`` that is not finite and
        > 0, on a ladder engine and from ``temp == 0``; ``NotImplementedError`` with ``reference_energy_ledgers=True``."""
        temp = float(temp)
        if not (np.isfinite(temp) and temp > 0):
            raise ValueError("the new temperature must be finite and > 0")
        if self.temperatures is not None:
            raise ValueError("population annealing needs the scalar temp: this engine has a temperature ladder")
        if not self.temp > 0:
            raise ValueError("population annealing cannot reweight from temp = 0: set_temp first")
        self._check(self._lib.me_population_resample(self._handle, temp))
        self.temp = temp
        self._population_used = True

    def _reset_population(self):
        """Back to the state before any set_temp / resample: the constructor's temp, no stages, families = global ids."""
        self._check(self._lib.me_set_temperature(self._handle, float(self._initial_temp)))
        self.temp = self._initial_temp
        self._check(self._lib.me_set_population_stats(self._handle, 0, None, None, None, None))
        ids = np.arange(self.n_chains, dtype=np.int64) + np.int64(self.chain_offset)
        self._check(self._lib.me_set_population_families(self._handle, 0, self.n_chains,
                                                         ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        self._population_used = False

    def anneal(self, temps, n_sweeps=1):
        """For each ``T`` of ``temps`` in turn: :meth:`resample` to ``T``, then ``step_all(n_sweeps)``.

        The proposal widths are not touched: they stay with the slots and adapt only as :meth:`step_all` adapts them, by
        about 1/200 per step.  Over a large cooling that is too slow for a many-dimensional space -- proposals far wider
        than the cold Boltzmann width are almost all rejected, the population stops moving between stages and ``log_z``
        comes out biased low (a 16-dimensional quadratic cooled a hundredfold in 40 stages of 10 sweeps: 1-2 too low).
        Start from a population equilibrated at the first temperature, and where the energy is close to quadratic scale
        the widths by ``sqrt(T_new / T_old)`` at each stage (``tests/test_gpu_population.py``, ``_anneal_quadratic``) or
        give each stage enough sweeps for the adaptation to follow."""
        for t in np.asarray(temps, dtype=np.float64).ravel():
            self.resample(t)
            self.step_all(n_sweeps)

    def population_stats(self):
        """The stages so far: ``{"stages": int, "temps", "log_weight", "neff_fraction", "n_finite", "log_z"}`` -- per stage its
        new temperature, the estimate of ``ln Z(T_k) / Z(T_{k-1})``, ``W^2 / (N S2)``, the chains of finite weight, and
        ``log_z`` = the running sum of ``log_weight`` (``ln Z(T_k) / Z(T_start)``)."""
        stages = ctypes.c_uint64()
        self._check(self._lib.me_population_stats(self._handle, ctypes.byref(stages), None, None, None, None, 0))
        k = stages.value
        temps, lw, neff = (np.empty(k, dtype=np.float64) for _ in range(3))
        nfin = np.empty(k, dtype=np.int64)
        if k:
            self._check(self._lib.me_population_stats(self._handle, ctypes.byref(stages), _as_double_ptr(temps),
                                                      _as_double_ptr(lw), _as_double_ptr(neff),
                                                      nfin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), k))
        return {"stages": k, "temps": temps, "log_weight": lw, "neff_fraction": neff, "n_finite": nfin,
                "log_z": np.cumsum(lw)}

    def families(self):
        """The family id of every local chain, ``(n_chains,)`` int64: the global chain id of its founder (``chain_offset + j``
        before the first stage).  Resampling keeps the array non-decreasing."""
        out = np.empty(self.n_chains, dtype=np.int64)
        self._check(self._lib.me_population_families(self._handle, 0, self.n_chains,
                                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def n_families(self):
        """The number of surviving families, ``1 + #{j : fam[j] != fam[j-1]}``."""
        fam = self.families()
        return int(1 + np.count_nonzero(fam[1:] != fam[:-1]))

    # -- RCCL behind the C ABI (me_comm_*): the all-reduce of the moments runs on the engine's own streams, no PyTorch
    @staticmethod
    def comm_unique_id():
        """Rank 0: a fresh ``ncclUniqueId`` (bytes) to hand to every rank's :meth:`comm_init`."""
        buf = ctypes.create_string_buffer(_capi.COMM_ID_BYTES)
        _capi.check(_capi.load().me_comm_unique_id(buf, _capi.COMM_ID_BYTES))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """Join the RCCL communicator named by ``unique_id`` as ``rank`` of ``world`` (collective over all ranks)."""
        uid = bytes(unique_id)
        if len(uid) != _capi.COMM_ID_BYTES:
            raise ValueError("the unique id is %d bytes" % _capi.COMM_ID_BYTES)
        self._check(self._lib.me_comm_init_rank(self._handle, uid, len(uid), int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._lib.me_comm_destroy(self._handle))

    def comm_info(self):
        """(rank, world, RCCL version code); (-1, 0, 0) without a communicator."""
        rank, world, version = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.me_comm_info(self._handle, ctypes.byref(rank), ctypes.byref(world), ctypes.byref(version)))
        return rank.value, world.value, version.value

    def pooled_moments_allreduce(self):
        """Ensemble sums over ALL ranks' chains: reduction kernels, ``ncclAllReduce`` and the copy to the host enqueued on
        the engine's streams; waits for the copy only."""
        size = ctypes.c_int64()
        self._check(self._lib.me_pooled_moments_size(self._handle, ctypes.byref(size)))
        out = np.empty(size.value, dtype=np.float64)
        self._check(self._lib.me_pooled_moments_allreduce(self._handle, _as_double_ptr(out), size.value))
        return out

    def pooled_moments_allreduce_begin(self):
        """The same without waiting; collect with :meth:`pooled_moments_end`."""
        self._check(self._lib.me_pooled_moments_allreduce_begin(self._handle))

    def pooled_moments_into(self, device_ptr, n_doubles):
        """Write the local ensemble sums into caller-owned device memory (e.g. a torch CUDA tensor's data_ptr)."""
        self._check(self._lib.me_pooled_moments_device(self._handle, ctypes.c_void_p(device_ptr), int(n_doubles)))

    def shared_factor(self):
        """The packed factor last installed with :meth:`set_shared_factor`, or ``None``."""
        nr, nc = self.num_real_params, self.num_complex_params
        out = np.empty(nr * (nr + 1) // 2 + nc * nc, dtype=np.float64)
        is_set = ctypes.c_int32()
        self._check(self._lib.me_get_shared_factor(self._handle, _as_double_ptr(out), out.size, ctypes.byref(is_set)))
        return out if is_set.value else None

    def set_shared_factor(self, packed_factor):
        f = np.ascontiguousarray(packed_factor, dtype=np.float64)
        self._check(self._lib.me_set_shared_factor(self._handle, _as_double_ptr(f), f.size))

    def time_steps(self, n_launches, n_sweeps=1):
        """Device milliseconds (HIP events on the engine's stream) of ``n_launches`` step launches."""
        ms = ctypes.c_float()
        self._check(self._lib.me_time_steps(self._handle, int(n_launches), int(n_sweeps), ctypes.byref(ms)))
        return ms.value

    def proposal_factors(self):
        """Per-chain Cholesky factors the next proposals use: (real [n,nr,nr], complex [n,nc,nc])."""
        packed = self._get(_capi.FIELD_FACTOR)
        nr, nc = self.num_real_params, self.num_complex_params
        return unpack_real_factor(packed, nr), unpack_complex_block(packed, nr, nc, hermitian=False)

    # ------------------------------------------------------------------ checkpoint (the reference has only the
    # constructor warm start, metropolis_engine.py:17,24)
    _STATE_FIELDS = (("params", _capi.FIELD_PARAMS), ("energy", _capi.FIELD_ENERGY), ("width", _capi.FIELD_WIDTH),
                     ("mean", _capi.FIELD_MEAN), ("obs_mean", _capi.FIELD_OBS_MEAN), ("cov", _capi.FIELD_COV),
                     ("factor", _capi.FIELD_FACTOR), ("energy_total", _capi.FIELD_ENERGY_TOTAL))

    def state_dict(self):
        state = {}
        for name, field in self._STATE_FIELDS:
            try:
                state[name] = self._get(field)
            except NotImplementedError:
                pass
        step, meas = self._counters()
        state["step_index"], state["measure_step_counter"] = step, meas
        state["uses_per_chain_factors"] = bool(meas > 50 and self.cov_mode == "reference")
        state["accepted"], state["proposed"] = self.accept_stats()
        shared = self.shared_factor()
        if shared is not None:                       # cov_mode="pooled": the proposal shape every chain shares
            state["shared_factor"] = shared
        temps = self.temperatures
        if temps is not None:                        # a ladder engine: the ladder and the replica-exchange position
            state["temperatures"] = temps
            state["replica_round"], state["swap_attempted"], state["swap_accepted"] = self.swap_stats()
        if self._population_used:                    # set_temp / resample: the temperature, the stages and the families
            stats = self.population_stats()
            state["temp"] = float(self.temp)
            for key in ("temps", "log_weight", "neff_fraction", "n_finite"):
                state["population_" + key] = stats[key]
            state["families"] = self.families()
        return state

    def load_state_dict(self, state):
        """Restore a :meth:`state_dict`.  Everything is validated against THIS engine before the first device write -- a
        checkpoint of an engine with other fields (e.g. ``reference_energy_ledgers=True``, a tracked covariance, a shared
        factor) or other shapes raises and leaves the engine untouched."""
        todo = []
        for name, field in self._STATE_FIELDS:
            if name in state and (name != "factor" or state.get("uses_per_chain_factors", False)):
                comps = ctypes.c_int32()
                self._check(self._lib.me_field_components(self._handle, field, ctypes.byref(comps)))   # NotImplementedError
                values = np.asarray(state[name], dtype=np.float64)
                if values.shape != (self.n_chains, comps.value):
                    raise ValueError("checkpoint field %r has shape %s, this engine keeps %s"
                                     % (name, values.shape, (self.n_chains, comps.value)))
                todo.append((field, values))
        if "step_index" not in state or "measure_step_counter" not in state:
            raise ValueError("checkpoint lacks the step / measure counters")
        if int(state["measure_step_counter"]) < 1:
            raise ValueError("measure_step_counter starts at 1")
        if "shared_factor" in state:
            nr, nc = self.num_real_params, self.num_complex_params
            if self.cov_mode != "pooled":
                raise ValueError("the checkpoint carries a shared proposal factor: this engine needs cov_mode='pooled'")
            if np.asarray(state["shared_factor"]).shape != (nr * (nr + 1) // 2 + nc * nc,):
                raise ValueError("checkpoint shared_factor has the wrong length")
        if "accepted" in state and "proposed" in state and int(state["accepted"]) > int(state["proposed"]):
            raise ValueError("checkpoint accept counters are inconsistent")
        population = None
        if "temp" in state:
            temp = float(state["temp"])
            if not (np.isfinite(temp) and temp >= 0):
                raise ValueError("checkpoint temp must be finite and >= 0")
            if "temperatures" in state:
                raise ValueError("the checkpoint carries both a scalar temp and a temperature ladder")
            keys = ("population_temps", "population_log_weight", "population_neff_fraction", "population_n_finite")
            if any(key not in state for key in keys) or "families" not in state:
                raise ValueError("checkpoint lacks the population stages / families of its temp")
            temps, lw, neff = (np.ascontiguousarray(state[key], dtype=np.float64) for key in keys[:3])
            nfin = np.ascontiguousarray(state[keys[3]], dtype=np.int64)
            if not (temps.ndim == 1 and lw.shape == neff.shape == nfin.shape == temps.shape):
                raise ValueError("checkpoint population stages must be 1-D arrays of one length")
            if not np.all(np.isfinite(temps) & (temps > 0)) or np.any(nfin < 0) or np.any(nfin > self.n_chains):
                raise ValueError("checkpoint population stages are inconsistent")
            fam = np.ascontiguousarray(state["families"], dtype=np.int64)
            if fam.shape != (self.n_chains,):
                raise ValueError("checkpoint families must hold one id per chain")
            population = (temp, temps, lw, neff, nfin, fam)
        # a checkpoint without "temp" was taken before set_temp / resample were used: the engine returns to its constructor's
        # temp, no stages and every chain its own family, so that its history and the checkpoint's do not mix
        reset_population = population is None and self._population_used
        ladder = None
        if "temperatures" in state:
            if (self._initial_temp if reset_population else self.temp) != 0:
                raise ValueError("the checkpoint carries a temperature ladder: this engine has a scalar temp")
            ladder = validate_ladder(state["temperatures"], self.n_chains)
            if "replica_round" not in state or "swap_attempted" not in state or "swap_accepted" not in state:
                raise ValueError("checkpoint lacks the replica-exchange round / swap counters of its ladder")
            att = np.asarray(state["swap_attempted"], dtype=np.int64)
            acc = np.asarray(state["swap_accepted"], dtype=np.int64)
            if att.shape != (ladder.size - 1,) or acc.shape != (ladder.size - 1,):
                raise ValueError("checkpoint swap counters must have one entry per adjacent pair of rungs")
            if np.any(acc < 0) or np.any(acc > att) or int(state["replica_round"]) < 0:
                raise ValueError("checkpoint swap counters are inconsistent")
        if reset_population:
            self._reset_population()
        if ladder is not None:
            # (first, so that an engine that cannot carry a ladder refuses before anything else is written)
            self.set_temperatures(ladder)
        for field, values in todo:
            self._set(field, values)
        self._check(self._lib.me_set_counters(self._handle, int(state["step_index"]),
                                              int(state["measure_step_counter"])))
        if "shared_factor" in state:
            self.set_shared_factor(state["shared_factor"])
        if "accepted" in state and "proposed" in state:
            self._check(self._lib.me_set_accept_stats(self._handle, int(state["accepted"]), int(state["proposed"])))
        if ladder is not None:
            n_pairs = ladder.size - 1
            att = (ctypes.c_uint64 * max(n_pairs, 1))(*[int(v) for v in state["swap_attempted"]])
            acc = (ctypes.c_uint64 * max(n_pairs, 1))(*[int(v) for v in state["swap_accepted"]])
            self._check(self._lib.me_set_replica_stats(self._handle, int(state["replica_round"]), att, acc, n_pairs))
        if population is not None:
            temp, temps, lw, neff, nfin, fam = population
            if self.temperatures is not None:          # a scalar-temperature checkpoint replaces a ladder
                self.set_temperatures(None)
            self.set_temp(temp)
            self._check(self._lib.me_set_population_stats(self._handle, temps.size, _as_double_ptr(temps), _as_double_ptr(lw),
                                                          _as_double_ptr(neff),
                                                          nfin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            self._check(self._lib.me_set_population_families(self._handle, 0, self.n_chains,
                                                             fam.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))

    # ------------------------------------------------------------------ time series (:31-35, :350-356, :466-479)
    def trace(self):
        """Recorded series as ``[n_measures, n_traced, D + n_terms + n_widths]``: params, energy terms, widths per
        measure()."""
        rows, cols, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.me_trace_shape(self._handle, ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(k)))
        out = np.empty((rows.value, cols.value, k.value), dtype=np.float64)
        self._check(self._lib.me_trace_get(self._handle, _as_double_ptr(out), out.size))
        return np.ascontiguousarray(out.transpose(0, 2, 1))

    def _series(self, chain=0):
        tr = self.trace()
        if tr.shape[1] <= chain:
            raise ValueError("chain %d is not traced (trace_chains=%d)" % (chain, self.trace_chains))
        tr = tr[:, chain, :]
        nr, nc = self.num_real_params, self.num_complex_params
        d = nr + 2 * nc
        real = tr[:, :nr]
        cplx = tr[:, nr:nr + nc] + 1j * tr[:, nr + nc:d]
        obs = np.concatenate((np.abs(real), np.abs(cplx), real ** 2), axis=1)
        t = len(self.energy_term_names)
        widths = tr[:, d + t:]
        w_real = widths[:, 1 if widths.shape[1] == 3 else 0] if nr else None
        w_cplx = widths[:, 2 if widths.shape[1] == 3 else 0] if nc else None
        return real, cplx, obs, tr[:, d:d + t], w_real, w_cplx

    @property
    def real_params_time_series(self):
        return list(self._series()[0]) if self.num_real_params else None                  # :48

    @property
    def complex_params_time_series(self):
        return list(self._series()[1]) if self.num_complex_params else None               # :58

    @property
    def observables_time_series(self):
        return list(self._series()[2])

    @property
    def energy_time_series(self):
        series = self._series()[3]
        return {name: list(series[:, t]) for t, name in enumerate(self.energy_term_names)}            # :123

    @property
    def real_group_sampling_width_time_series(self):
        return list(self._series()[4]) if self.num_real_params else None

    @property
    def complex_group_sampling_width_time_series(self):
        return list(self._series()[5]) if self.num_complex_params else None

    def time_series_frame(self, chain=0):
        """The reference's DataFrame layout (metropolis_engine.py:466-478; column order of exampledata.csv:1) for one
        traced chain: observables, ``<term>_energy``, real parameters, ``real_group_sampling_width``, complex
        parameters, ``complex_group_sampling_width``."""
        import pandas
        real, cplx, obs, energy, w_real, w_cplx = self._series(chain)
        nr, nc = self.num_real_params, self.num_complex_params
        cols = {}
        for i, name in enumerate(self.observables_names):
            cols[name] = obs[:, i]
        for name in sorted(self.energy_term_names):    # one column per energy term (:468-469; the reference iterates a set)
            cols[name + "_energy"] = energy[:, self.energy_term_names.index(name)]
        if nr:
            for i in range(nr):
                cols[self.params_names[i]] = real[:, i]
            cols["real_group_sampling_width"] = w_real
        if nc:
            for i in range(nc):
                cols[self.params_names[nr + i]] = cplx[:, i]
            cols["complex_group_sampling_width"] = w_cplx
        return pandas.DataFrame.from_dict(cols)

    def save_time_series(self):
        self.df = self.time_series_frame(0)
        print(self.df)                                                                   # :479

    def equilibration_points(self, fast=True, nskip=1):
        """Equilibration start, statistical inefficiency and effective sample count of EVERY traced chain and recorded
        column in one GPU batch (``me_detect_equilibration``): ``{column: (t0[k], g[k], Neff[k])}`` over the ``k`` traced
        chains.  The many-chain form of ``get_equilibration_points`` (statistics.py:25-48); PARITY UNPINNED like it."""
        from . import statistics
        names, rows = [], []
        for chain in range(self.trace_chains):
            frame = self.time_series_frame(chain)
            if chain == 0:
                for name in frame.columns.values:
                    values = frame[name].to_numpy()
                    names += [name + "_real", name + "_imag"] if np.iscomplexobj(values) else [name]
            for name in frame.columns.values:
                values = frame[name].to_numpy()
                rows += [values.real, values.imag] if np.iscomplexobj(values) else [values.astype(np.float64)]
        t0, g, neff = statistics.detect_equilibration_batch(np.stack(rows), fast=fast, nskip=nskip, device=self.device)
        k, c = self.trace_chains, len(names)
        t0, g, neff = t0.reshape(k, c), g.reshape(k, c), neff.reshape(k, c)
        return {name: (t0[:, i], g[:, i], neff[:, i]) for i, name in enumerate(names)}

    def save_equilibrium_stats(self, external_df=None):
        """metropolis_engine.py:481-504: equilibration point per recorded column, the global cut-off (largest ``t0``
        over the columns that are not sampling widths) and the re-averaged means.  PARITY UNPINNED: the reference
        delegates to pymbar, which is absent; see metropolisengine_amd/statistics.py."""
        import pandas
        from . import statistics
        if self.df is None:
            self.save_time_series()
        if external_df is not None:
            frames = [self.df] + [df for df in external_df if isinstance(df.iloc[0, 0], (float, int))]   # :486
            all_df = pandas.concat(frames, axis=1)
        else:
            all_df = self.df
        self.eq_points = statistics.get_equilibration_points(all_df)
        self.global_eq_point = max(t for key, (t, _, _) in self.eq_points.items() if "sampling_width" not in key)
        self.equilibrated_means, self.eq_means_error = statistics.get_equilibrated_means(self.df,
                                                                                         cutoff=self.global_eq_point)
        if external_df is not None:
            profiles = [statistics.get_equilibrated_means(e_df, cutoff=self.global_eq_point)[0] for e_df in external_df]
            self.field_profile = profiles[0]                                             # :501-502
            if len(profiles) > 1:
                self.field_abs_profile = profiles[1]
        print("global t_0", self.global_eq_point)                                        # :503
        self.equilibrated_means["global_cutoff"] = self.global_eq_point
