"""A corpus of Python energies and reject conditions written the way a user of the reference writes them (test data only):
numpy idioms on ``real_params`` (float64 array) and ``complex_params`` (complex128 array), each with the parameter shape it
is written for, the input domain on which it is defined and well scaled, and whether metropolisengine_amd/pyenergy.py must
TRACE it or REFUSE it with a TraceError.

Used by tests/test_pyenergy_corpus_cpu.py (graph against callable, refusals, the emitter compiled for the host) and
tests/test_gpu_pyenergy_corpus.py (the traceable energies packed into one term-dictionary plugin per shape, on the GPU).
The plugins are built by ``__graft_entry__.build()`` (``PLUGINS``), so the two sides must see identical callables."""
import math
from collections import namedtuple

import numpy as np

Domain = namedtuple("Domain", "name lo hi")
ANY = Domain("any", -1e3, 1e3)              # every real / imaginary part in [-1e3, 1e3]
BOUNDED = Domain("bounded", -2.0, 2.0)      # exp, sinh, cosh, 2**x: no float32 overflow
POSITIVE = Domain("positive", 1e-8, 1e3)    # log, real powers, negative powers

# kind: "energy" (a callable), "dict" (the reference's {"all", "real", "complex"} term dictionary) or "reject"
Entry = namedtuple("Entry", "name shape fn domain expect kind")

_ENTRIES = []


def _energy(name, shape, domain=ANY, expect="trace"):
    def add(fn):
        _ENTRIES.append(Entry(name, shape, fn, domain, expect, "energy"))
        return fn
    return add


def _reject(name, shape, domain=ANY, expect="trace"):
    def add(fn):
        _ENTRIES.append(Entry(name, shape, fn, domain, expect, "reject"))
        return fn
    return add


K3 = np.array([[2.0, 0.3, -0.1], [0.3, 1.0, 0.2], [-0.1, 0.2, 0.5]])
W3 = np.array([0.5, -1.25, 2.0])
W7 = np.linspace(0.5, 2.0, 7)

# ============================================================================ shape (3, 0): three real parameters
_energy("quadratic_form", (3, 0))(lambda r, c: r @ K3 @ r)
_energy("sum_mean_var", (3, 0))(lambda r, c: np.sum(r ** 2) + np.mean(r) ** 2 + 3.0 * np.var(r))
_energy("prod_and_python_sum_abs", (3, 0))(lambda r, c: np.prod(r) + sum(abs(v) for v in r) + abs(r[0] - r[2]))
_energy("slices_broadcast", (3, 0))(lambda r, c: np.sum(W3 * r ** 2) + np.sum((r[1:] - r[:-1]) ** 2) + np.dot(W3[::-1], r))
_energy("real_imag_of_real_array", (3, 0))(lambda r, c: np.sum(r.real ** 2) + np.sum(r.imag) + np.sum(np.real(r) * np.imag(r)))
_energy("int_powers", (3, 0))(lambda r, c: r[0] ** 3 - 2.0 * r[1] ** 4 + r[2] ** 6 / 64.0 + r[0] ** 2 * r[1] ** 5)
_energy("neg_int_and_real_powers", (3, 0))(
    lambda r, c: (r[0] ** 2 + 0.25) ** -3 + 2.0 * (1.0 + r[1] ** 2) ** -2 + np.abs(r[2]) ** 1.5 + np.abs(r[0]) ** 0.5
    + np.sum((r ** 2 + 1e-3) ** 1.125))
_energy("log_sqrt", (3, 0))(
    lambda r, c: np.sum(np.log(r ** 2 + 1e-3)) + np.sqrt(np.abs(r[0] * r[1])) - np.log(np.abs(r[2]) + 1.0))
_energy("exp_pow2_sinh_cosh", (3, 0), BOUNDED)(
    lambda r, c: np.sum(np.exp(-r ** 2)) + 2 ** r[0] + np.sinh(r[1]) * np.cosh(r[2]) + 0.5 ** r[2])
_energy("trig_sums_products", (3, 0))(
    lambda r, c: np.sin(r[0]) * np.cos(r[1]) + np.cos(r[0]) * np.sin(r[1]) + np.sum(np.cos(r) ** 2) * np.arctan(r[2]))
_energy("tan_tanh_arctan2", (3, 0), BOUNDED)(
    lambda r, c: np.tan(r[0]) * np.tanh(r[1]) + np.arctan2(r[1], r[2]) + np.tanh(r[2]) ** 2 - np.tan(0.5 * r[1]))
_energy("shared_subexpressions", (3, 0), BOUNDED)(
    lambda r, c: _shared(r[0], r[1], r[2]))


def _shared(a, b, c):
    """One subexpression used many times over (CSE): the emitter writes it once."""
    s = a * a + b * b + c * c
    u = np.exp(-s) * s + np.sin(s) * np.cos(s)
    v = (u + s) * (u - s) + u * s
    return v + s ** 2 * u + np.sqrt(1.0 + s) * (u + v) - np.tanh(u * v + s)


# ============================================================================ shape (0, 3): three complex parameters
_energy("re2_plus_im2", (0, 3))(lambda r, c: np.sum(c.real ** 2 + c.imag ** 2))
_energy("np_real_np_imag", (0, 3))(lambda r, c: np.sum(np.real(c) ** 2 + 3.0 * np.imag(c) ** 2) + np.sum(np.imag(c)))
_energy("imag_linear_and_cubic", (0, 3))(lambda r, c: np.sum(c.imag) + np.sum(c.imag ** 3) - np.sum(c.real) * c.imag[0])
_energy("conj_forms", (0, 3))(
    lambda r, c: np.sum((c * c.conj()).real) ** 2 + np.sum(np.conj(c) * c[::-1]).real + (c.conjugate()[0] * c[1]).imag)
_energy("abs_square_and_square", (0, 3))(
    lambda r, c: np.sum(np.abs(c) ** 2) + np.sum(np.square(c)).real + np.sum(np.abs(c) ** 4) - np.sum(np.square(c.imag)))
_energy("powers_of_derived", (0, 3))(lambda r, c: np.sum((c ** 2).imag ** 2) + np.sum((c ** 3).real) + ((c[0] + 2.0) ** -1).real)
_energy("angle_arctan2", (0, 3))(
    lambda r, c: np.sum(np.arctan2(c.imag, c.real) ** 2) + np.sum(np.cos(np.angle(c))) + np.angle(c[1:], deg=True)[0])
_energy("vdot_dot_matmul_einsum", (0, 3))(
    lambda r, c: np.vdot(c, c).real + np.dot(c, c).imag + (c @ c.conj()).real + np.einsum("i,i", c, np.conj(c)).real)
_energy("complex_constants", (0, 3))(
    lambda r, c: np.sum(((1.0 - 2.0j) * c + 0.5j).real ** 2) + (np.array([1j, -1.0, 0.5 + 0.5j]) @ c).imag)
_energy("complex_division", (0, 3))(lambda r, c: np.sum((1.0 / (1.0 + c * c.conj())).real) + ((c[0] + 2.0) / (c[1] + 3.0)).imag)
_energy("log_of_modulus", (0, 3))(lambda r, c: np.sum(np.log(1.0 + np.abs(c) ** 2)) + np.log(1.0 + c.real[0] ** 2))
_energy("mean_var_of_complex", (0, 3))(lambda r, c: np.var(c) + np.abs(np.mean(c)) ** 2 + np.var(c.imag))

# ============================================================================ shape (2, 3): two real + three complex
_energy("landau_field", (2, 3))(
    lambda r, c: r[0] * r[1] * np.sum(-1.0 * c * c.conjugate() + 0.5 * c ** 2 * c.conjugate() ** 2).real)
_energy("mixed_re_im_real", (2, 3))(lambda r, c: np.sum(c.real ** 2 + c.imag ** 2) * (1.0 + r[0] ** 2) + r[1] * np.sum(c.imag))
_energy("mixed_np_real_imag", (2, 3))(lambda r, c: np.sum(np.real(c) * r[0] - np.imag(c) * r[1]) ** 2 + np.sum(r ** 2))
_energy("mixed_angle", (2, 3))(lambda r, c: np.sum(np.sin(np.angle(c) - r[0]) ** 2) + np.cos(r[1]) * np.abs(c[0]))
_energy("mixed_arctan2", (2, 3))(lambda r, c: np.sum(np.arctan2(c.imag + r[0], c.real - r[1])) + np.arctan(r[0] * r[1]))
_energy("mixed_exp_sqrt", (2, 3), BOUNDED)(
    lambda r, c: np.exp(-np.sum(np.abs(c) ** 2)) * np.sqrt(1.0 + r[0] ** 2) + np.exp(r[1]) * np.sum(c.real))
_energy("mixed_tanh_sinh_cosh", (2, 3), BOUNDED)(
    lambda r, c: np.tanh(np.sum(c.imag)) * np.sinh(r[0]) + np.cosh(r[1]) * np.sum(np.tanh(c.real) ** 2))
_energy("mixed_log", (2, 3))(lambda r, c: np.log(1.0 + r[0] ** 2 + np.sum(np.abs(c) ** 2)) * (r[1] ** 2 + 0.5))
_energy("mixed_vdot_conj", (2, 3))(lambda r, c: r[0] * np.vdot(c, c[::-1]).real + r[1] * (c * np.conj(c)).real.sum())
_energy("mixed_tan_pow", (2, 3), BOUNDED)(lambda r, c: np.tan(0.5 * r[0]) * np.sum(c.imag ** 2) + 2 ** r[1] * np.abs(c[2]) ** 2)
_energy("mixed_prod_mean", (2, 3))(lambda r, c: np.prod(np.abs(c)) + np.mean(c.real * r[0]) + np.prod(r) * np.mean(c.imag))

# ============================================================================ shape (2, 7): D = 16, tile-major state
_energy("cylinder_like", (2, 7))(
    lambda r, c: np.sum(W7 * np.abs(c) ** 2) * (r[0] - 1.0) ** 2 + np.sum(np.abs(c) ** 4) + r[1] ** 2)
_energy("wide_re_im", (2, 7))(lambda r, c: np.sum(c.real ** 2 - 0.5 * c.imag ** 2) + np.sum(c.imag ** 2) * r[0])
_energy("wide_neighbours", (2, 7))(lambda r, c: np.sum(np.abs(c[1:] - c[:-1]) ** 2) + (c[0] * c[-1].conj()).real * r[1])
_energy("wide_angle_var", (2, 7))(lambda r, c: np.var(np.angle(c)) + np.mean(np.cos(np.angle(c) * 2.0)) * r[0])
_energy("wide_einsum_dot", (2, 7))(lambda r, c: np.einsum("i,i", W7, np.abs(c) ** 2) + np.dot(W7, c.imag) * np.dot(r, r))
_energy("wide_log_sqrt", (2, 7))(
    lambda r, c: np.sum(np.log(np.abs(c) ** 2 + 1e-2)) + np.sqrt(np.abs(r[0] * r[1])) + np.sum(np.sqrt(np.abs(c.real * c.imag))))
_energy("wide_real_powers", (2, 7))(
    lambda r, c: np.sum(np.abs(c.real) ** 1.25) + (r[0] ** 2 + 0.5) ** -2 + np.sum((c.imag ** 2 + 1.0) ** -1.0))

# ============================================================================ CPU only: defined on positive arguments alone
# (the engine refuses a non-finite energy, and its moves would leave the domain)
_energy("log_and_powers_of_positive", (1, 1), POSITIVE)(
    lambda r, c: np.log(r[0]) + np.log(np.abs(c[0])) + r[0] ** -2.5 + c.real[0] ** 1.5 + c.imag[0] ** -3)
_energy("wide_exp", (2, 7), BOUNDED)(lambda r, c: np.sum(np.exp(c.real - c.imag)) + np.exp(-r[0] ** 2) * np.sum(np.cos(c.imag)))
_energy("wide_trig", (2, 7))(lambda r, c: np.sum(np.sin(c.real) * np.cos(c.imag)) + np.sum(np.arctan(c.real * r[1])))
_energy("wide_cosh_tanh", (2, 7), BOUNDED)(lambda r, c: np.sum(np.cosh(c.imag)) - np.sum(np.tanh(c.real)) * np.sinh(r[1]))
_energy("wide_conj_products", (2, 7))(
    lambda r, c: np.sum((c ** 2 * np.conj(c) ** 2).real) - np.sum((c * c.conjugate()).real) * (r[0] + r[1]))

# ============================================================================ must be refused with a TraceError
_energy("np_max", (3, 0), expect="refuse")(lambda r, c: np.max(r ** 2))
_energy("np_where", (3, 0), expect="refuse")(lambda r, c: np.sum(np.where(r > 0, r, -2.0 * r)))
_energy("np_clip", (3, 0), expect="refuse")(lambda r, c: np.sum(np.clip(r, -1.0, 1.0) ** 2))
_energy("np_sign", (3, 0), expect="refuse")(lambda r, c: np.sum(np.sign(r) * r))
_energy("chained_comparison", (3, 0), expect="refuse")(lambda r, c: r[0] ** 2 if 0.0 < r[0] < 1.0 else 1.0)
_energy("np_any", (3, 0), expect="refuse")(lambda r, c: np.sum(r ** 2) + 10.0 * np.any(r > 2.0))
_energy("np_all", (0, 3), expect="refuse")(lambda r, c: np.sum(np.abs(c)) * np.all(np.abs(c) < 1.0))
_energy("math_exp", (3, 0), expect="refuse")(lambda r, c: math.exp(r[0]))
_energy("math_sqrt", (0, 3), expect="refuse")(lambda r, c: math.sqrt(np.sum(np.abs(c) ** 2)))
_energy("complex_exp", (0, 3), expect="refuse")(lambda r, c: np.sum(np.exp(c)).real)
_energy("complex_norm", (0, 3), expect="refuse")(lambda r, c: np.linalg.norm(c))
_energy("log1p", (3, 0), expect="refuse")(lambda r, c: np.log1p(r[0] ** 2))
_energy("expm1", (3, 0), expect="refuse")(lambda r, c: np.expm1(r[0]))
_energy("hypot", (3, 0), expect="refuse")(lambda r, c: np.hypot(r[0], r[1]))
_energy("python_float", (3, 0), expect="refuse")(lambda r, c: float(r[0]) ** 2)
_energy("complex_real_power", (0, 3), expect="refuse")(lambda r, c: np.sum(c ** 0.5).real)
_energy("returns_an_array", (3, 0), expect="refuse")(lambda r, c: r ** 2)

# ============================================================================ reject conditions
_reject("abs_wall", (2, 3))(lambda r, c: abs(r[0]) >= 1.5)
_reject("box_on_all_parts", (2, 3))(
    lambda r, c: (np.abs(r[0]) >= 1.5) | (np.abs(r[1]) >= 1.5) | (np.sum(c.real ** 2 + c.imag ** 2) >= 9.0))
_reject("disc", (3, 0))(lambda r, c: r[0] ** 2 + r[1] ** 2 > 4.0)
_reject("modulus", (0, 3))(lambda r, c: np.abs(c[0]) > 2.0)
_reject("negated", (3, 0))(lambda r, c: ~(r[0] < 0.5))
_reject("real_or_imag", (0, 3))(lambda r, c: (c.real[0] > 1.0) | (c.imag[1] < -1.0))
_reject("angle_window", (0, 3))(lambda r, c: (np.angle(c)[0] > 2.5) & (np.abs(c[0]) > 0.1))
_reject("quadrant", (3, 0))(lambda r, c: (r[0] > 0) & (r[1] > 0))
_reject("sum_threshold", (2, 7))(lambda r, c: np.sum(np.abs(c) ** 2) + r[0] >= 20.0)
_reject("chained_comparison", (3, 0), expect="refuse")(lambda r, c: -1.0 < r[0] < 1.0)
_reject("np_any", (3, 0), expect="refuse")(lambda r, c: np.any(np.abs(r) > 1.0))
_reject("np_all", (0, 3), expect="refuse")(lambda r, c: np.all(np.abs(c) < 2.0))
_reject("python_or", (3, 0), expect="refuse")(lambda r, c: abs(r[0]) >= 1 or abs(r[1]) >= 1)
_reject("python_and", (3, 0), expect="refuse")(lambda r, c: r[0] > 1 and r[1] > 1)


# ============================================================================ term dictionaries ({"all", "real", "complex"})
def _landau_terms():
    field = lambda r, c: (r[0] * r[1] * (-1.0 * c * c.conjugate() + 0.5 * c ** 2 * c.conjugate() ** 2))[0]   # noqa: E731
    area = lambda r, c: (1 - r[0]) ** 2 + (1 - r[1]) ** 2                                                  # noqa: E731
    return {"complex": {"field": field}, "real": {"field": field, "area": area}, "all": {"field": field, "area": area}}


def _same_term_written_twice():
    """Two different callables under one name that compute the same thing: traced once, both checked."""
    a = lambda r, c: np.sum(c.real ** 2 + c.imag ** 2) + r[0] ** 2                                          # noqa: E731
    b = lambda r, c: np.sum(np.abs(c) ** 2) + r[0] * r[0]                                                   # noqa: E731
    return {"all": {"e": a}, "real": {"e": a}, "complex": {"e": b}}


def _groups_disagree():
    """the reference evaluates calc_energy[group][term] per group, so "real" and "complex" may hold different
    callables under one name; one device function cannot be both, so this must be refused."""
    real = lambda r, c: r[0] ** 2 + np.sum(np.abs(c) ** 2)                                                  # noqa: E731
    cplx = lambda r, c: 2.0 * np.sum(np.abs(c) ** 2)                                                        # noqa: E731
    return {"all": {"e": real}, "real": {"e": real}, "complex": {"e": cplx}}


_ENTRIES.append(Entry("landau_terms", (2, 1), _landau_terms(), ANY, "trace", "dict"))
_ENTRIES.append(Entry("same_term_written_twice", (1, 3), _same_term_written_twice(), ANY, "trace", "dict"))
_ENTRIES.append(Entry("groups_disagree", (1, 2), _groups_disagree(), ANY, "refuse", "dict"))

ENTRIES = tuple(_ENTRIES)
assert len({(e.kind, e.name) for e in ENTRIES}) == len(ENTRIES)


def entries(kind=None, expect=None, shape=None):
    return [e for e in ENTRIES if (kind is None or e.kind == kind) and (expect is None or e.expect == expect)
            and (shape is None or e.shape == shape)]


# ============================================================================ the GPU plugins: one per shape
GPU_SHAPES = ((3, 0), (0, 3), (2, 3), (2, 7))
GPU_REJECT = {(2, 3): "box_on_all_parts"}          # the plugin that carries a traced reject condition


def plugin_dictionary(shape):
    """Every traceable energy of ``shape`` as one term of a dictionary, listed in every group the shape has (so that any
    move, real-group or complex-group, recomputes every ledger row)."""
    terms = {e.name: e.fn for e in entries("energy", "trace", shape)}
    groups = {"all": terms}
    if shape[0]:
        groups["real"] = dict(terms)
    if shape[1]:
        groups["complex"] = dict(terms)
    return groups


def plugin_reject(shape):
    name = GPU_REJECT.get(shape)
    return None if name is None else next(e.fn for e in entries("reject", shape=shape) if e.name == name)


def plugin_domains(shape):
    """{term name: Domain} of the plugin's terms."""
    return {e.name: e.domain for e in entries("energy", "trace", shape)}


def plugin_domain(shape):
    """Where every term of the plugin is defined: the engine refuses a state at which any term is not finite."""
    domains = plugin_domains(shape).values()
    return Domain("plugin", max(d.lo for d in domains), min(d.hi for d in domains))


# (energy, n_real, n_complex, reject) of the GPU corpus plugins, built by __graft_entry__.build()
PLUGINS = tuple((plugin_dictionary(s), s[0], s[1], plugin_reject(s)) for s in GPU_SHAPES)


# ============================================================================ states
EDGE_VALUES = (0.0, 1.0, -1.0, 1e3, -1e3, 1e-8, -1e-8)


def random_states(domain, shape, n, rng):
    """``n`` random states of ``domain`` ([real | Re z | Im z] rows)."""
    d = shape[0] + 2 * shape[1]
    if domain.lo > 0:
        return np.exp(rng.uniform(-3.0, 3.0, size=(n, d)))
    if domain.hi < 10:
        return rng.uniform(domain.lo, domain.hi, size=(n, d))
    return rng.standard_normal((n, d)) * np.exp(rng.uniform(-2.0, 2.0, size=(n, 1)))


def edge_states(domain, shape, rng):
    """Every coordinate equal to each edge value inside ``domain``; and, where 0 is inside, purely imaginary complex
    parameters."""
    nr, nc = shape
    d = nr + 2 * nc
    edges = [np.full(d, v) for v in EDGE_VALUES if domain.lo <= v <= domain.hi]
    if nc and domain.lo <= 0.0 <= domain.hi:
        for _ in range(4):
            row = np.clip(rng.standard_normal(d), domain.lo, domain.hi)
            row[nr:nr + nc] = 0.0
            edges.append(row)
    return np.array(edges).reshape(-1, d)


def states(domain, shape, n_random, rng):
    """``n_random`` random states of ``domain`` and its edge states."""
    return np.vstack([random_states(domain, shape, n_random, rng), edge_states(domain, shape, rng)])


def in_domain(x, domain):
    return np.all((x >= domain.lo) & (x <= domain.hi), axis=-1)


def call(fn, x, shape):
    """The callable on numbers, as the reference calls it: float64 real_params, complex128 complex_params; the real part
    of a complex-typed result (the Landau toy's convention)."""
    nr, nc = shape
    with np.errstate(all="ignore"):
        out = fn(np.array(x[:nr], dtype=np.float64), x[nr:nr + nc] + 1j * x[nr + nc:])
    out = np.asarray(out).reshape(-1)[0] if isinstance(out, np.ndarray) else out
    return out if isinstance(out, (bool, np.bool_)) else complex(out).real
