"""Python energy callables on the GPU: the reference's ``energy(real_params, complex_params) -> float`` (and its energy
dictionaries, and ``reject_condition``) TRACED into a HIP device function and compiled around the kernels as a user plugin.

The reference couples sampler and physics through a Python callable that it invokes once per proposal
(metropolis_engine.py:20, :111-120, :250).  A HIP kernel cannot call Python, and this engine has no CPU fallback -- so the
callable is executed ONCE, at construction, on symbolic stand-ins for the parameters: ``real_params`` / ``complex_params`` are
numpy object arrays (:class:`SymArray`) of :class:`Sym` / :class:`SymComplex` nodes that overload arithmetic and record what
the function computes.  Whatever Python the function is written in -- lambdas, methods of a ``System`` object holding constants,
``*real_params`` unpacking, closures, helper functions, ``numpy`` ufuncs and reductions (the forms of README.md:26-33,
demo/toymodel_xypotentialwell.py:13-32 and demo/toymodel_complex_and_real.py:17-33) -- runs as ordinary Python; only
arithmetic on the parameters is recorded.  The recorded expression graph is written out as ``me_user_energy`` (straight-line
code, common subexpressions shared, sums of two products as explicit fused multiply-adds), compiled by hipcc
(``build.build_user_energy``) and loaded like any hand-written plugin (include/metropolis_user_energy.h).

What traces: ``+ - * /``, unary minus, ``abs``; integer powers (square and multiply), ``x ** 0.5`` (sqrt), real powers
and ``2 ** x`` (pow); ``np.sqrt``, ``np.exp``, ``np.log``, ``np.sin``, ``np.cos``, ``np.tan``, ``np.tanh``, ``np.sinh``,
``np.cosh``, ``np.arctan``, ``np.arctan2``, ``np.abs``, ``np.square`` on real values; complex ``+ - * /``, integer powers and
``abs``; element-wise ``.real``, ``.imag``, ``.conj()``, ``.conjugate()``, ``np.real``, ``np.imag``, ``np.conj`` and
``np.angle`` (``arctan2(im, re)``) on parameter arrays and on arrays computed from them; reductions and products that
numpy builds from these (``np.sum``, ``np.mean``, ``np.var``, ``np.prod``, ``np.dot``, ``np.vdot``, ``@``, ``np.einsum``,
Python ``sum``), slicing and broadcasting against constant arrays.  A ``reject_condition`` may compare traced values and
combine the comparisons with ``& | ~``.

What cannot be traced raises :class:`TraceError` at construction -- every exception raised while tracing is re-raised as
one, naming the original: control flow that depends on parameter VALUES (``if x > 0``, chained comparisons, ``max(x, y)``,
``np.max``, ``np.where``, ``np.clip``, ``np.sign``, ``np.any`` / ``np.all``, ``math.exp(x)`` -- use ``np.exp`` --,
``float(x)``), because the trace sees one symbolic evaluation, not one per chain; and numpy functions without a device
counterpart here (``np.log1p``, ``np.expm1``, ``np.hypot``, complex ``np.exp`` / ``np.log`` / ``np.sqrt``,
``np.linalg.norm`` of a complex array).  After tracing, the recorded graph is evaluated at 8 fixed-seed standard-normal
states (and the initial state, when the engine knows it) and compared with the callable on numbers -- for a term
dictionary, with every group's callable under each name: a difference beyond rounding is a :class:`TraceError` too, so an
idiom that records something other than what numpy computes cannot reach the GPU silently.
"""
import hashlib
import math
import os

import numpy as np

from . import _capi
from .energy import EnergySpec, RejectSpec

_UNARY = {"neg": "-({0})", "abs": "me_py_abs({0})", "sqrt": "me_py_sqrt({0})", "exp": "me_py_exp({0})", "log": "me_py_log({0})",
          "sin": "me_py_sin({0})", "cos": "me_py_cos({0})", "tan": "me_py_tan({0})", "tanh": "me_py_tanh({0})",
          "sinh": "me_py_sinh({0})", "cosh": "me_py_cosh({0})", "arctan": "me_py_atan({0})"}
_BINARY = {"add": "({0} + {1})", "sub": "({0} - {1})", "mul": "({0} * {1})", "div": "({0} / {1})", "pow": "me_py_pow({0}, {1})",
           "arctan2": "me_py_atan2({0}, {1})"}
_COMPARE = {"lt": "<", "le": "<=", "gt": ">", "ge": ">=", "eq": "==", "ne": "!="}


class TraceError(TypeError):
    """The Python energy does something that depends on parameter values and cannot be recorded symbolically."""


class Sym:
    """One real-valued node of the recorded expression graph: ``op`` in {"x", "const", unary, binary} with ``args``."""
    __array_priority__ = 1000.0
    __slots__ = ("op", "args", "value")

    def __init__(self, op, args=(), value=None):
        self.op, self.args, self.value = op, tuple(args), value

    # ---- construction helpers
    @staticmethod
    def lift(v):
        if isinstance(v, Sym):
            return v
        if isinstance(v, (bool, np.bool_)):
            raise TraceError("a boolean cannot be used as a number in a traced energy")
        if isinstance(v, (int, float, np.integer, np.floating)):
            return Sym("const", value=float(v))
        if isinstance(v, (complex, np.complexfloating)) and complex(v).imag == 0.0:
            return Sym("const", value=float(complex(v).real))
        raise TraceError("cannot use %r (%s) in a traced energy" % (v, type(v).__name__))

    def _bin(self, op, other, swap=False):
        if isinstance(other, (SymComplex, complex, np.complexfloating)) and not (
                isinstance(other, (complex, np.complexfloating)) and complex(other).imag == 0.0):
            return NotImplemented if isinstance(other, SymComplex) else SymComplex(self, Sym.lift(0.0))._bin(op, other, swap)
        if isinstance(other, np.ndarray):
            return NotImplemented
        a, b = (Sym.lift(other), self) if swap else (self, Sym.lift(other))
        if a.op == "const" and b.op == "const":              # constant folding keeps the generated code short
            return Sym("const", value={"add": a.value + b.value, "sub": a.value - b.value, "mul": a.value * b.value,
                                       "div": a.value / b.value if b.value else math.nan}[op])
        # identities that complex arithmetic with real constants produces by the dozen (x * (1 + 0j) = x + 0 i, ...)
        zero = lambda n: n.op == "const" and n.value == 0.0
        one = lambda n: n.op == "const" and n.value == 1.0
        if op == "mul":
            if zero(a) or zero(b):
                return Sym("const", value=0.0)
            if one(a):
                return b
            if one(b):
                return a
        elif op == "add":
            if zero(a):
                return b
            if zero(b):
                return a
        elif op == "sub":
            if zero(b):
                return a
            if zero(a):
                return -b
        elif op == "div" and one(b):
            return a
        return Sym(op, (a, b))

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("div", o)
    def __rtruediv__(self, o): return self._bin("div", o, True)
    def __neg__(self):
        if self.op == "const":
            return Sym("const", value=-self.value)
        return self.args[0] if self.op == "neg" else Sym("neg", (self,))

    def __pos__(self): return self
    def __abs__(self): return Sym("abs", (self,))

    def __pow__(self, o):
        if isinstance(o, (int, np.integer)) or (isinstance(o, (float, np.floating)) and float(o).is_integer() and abs(o) <= 64):
            n = int(o)
            if n == 0:
                return Sym.lift(1.0)
            out, base, k = None, self, abs(n)
            while k:                                           # square and multiply: x**4 is two multiplications
                if k & 1:
                    out = base if out is None else out * base
                k >>= 1
                if k:
                    base = base * base
            return out if n > 0 else 1.0 / out
        if isinstance(o, (float, np.floating)) and float(o) == 0.5:
            return Sym("sqrt", (self,))
        if isinstance(o, SymComplex):
            raise TraceError("complex exponents are not supported in a traced energy")
        return Sym("pow", (self, Sym.lift(o)))

    def __rpow__(self, o):
        return Sym("pow", (Sym.lift(o), self))

    # comparisons give boolean nodes (for reject_condition); using one in `if` / `and` / `or` is an error
    def _cmp(self, op, o): return SymBool("cmp", (self, Sym.lift(o)), op)
    def __lt__(self, o): return self._cmp("lt", o)
    def __le__(self, o): return self._cmp("le", o)
    def __gt__(self, o): return self._cmp("gt", o)
    def __ge__(self, o): return self._cmp("ge", o)
    def __eq__(self, o): return self._cmp("eq", o)
    def __ne__(self, o): return self._cmp("ne", o)
    __hash__ = object.__hash__

    def __float__(self):
        raise TraceError("the energy converts a parameter to a Python float (math.* functions, float(), int()): use the "
                         "numpy functions (np.exp, np.sqrt, ...) so that the computation can be recorded")
    __int__ = __index__ = __float__

    def __bool__(self):
        raise TraceError("the energy branches on a parameter value; a traced energy must be one arithmetic expression")

    # numpy object loops look these up by name (np.exp(x) -> x.exp())
    def conjugate(self): return self
    conj = conjugate
    real = property(lambda self: self)
    imag = property(lambda self: Sym.lift(0.0))
    def sqrt(self): return Sym("sqrt", (self,))
    def exp(self): return Sym("exp", (self,))
    def log(self): return Sym("log", (self,))
    def sin(self): return Sym("sin", (self,))
    def cos(self): return Sym("cos", (self,))
    def tan(self): return Sym("tan", (self,))
    def tanh(self): return Sym("tanh", (self,))
    def sinh(self): return Sym("sinh", (self,))
    def cosh(self): return Sym("cosh", (self,))
    def arctan(self): return Sym("arctan", (self,))
    def arctan2(self, o): return Sym("arctan2", (self, Sym.lift(o)))
    def square(self): return self * self
    def absolute(self): return abs(self)
    fabs = absolute


class SymBool:
    """A recorded comparison (or ``&`` / ``|`` / ``~`` of comparisons): the value of a traced ``reject_condition``."""
    __slots__ = ("op", "args", "cmp")

    def __init__(self, op, args, cmp=None):
        self.op, self.args, self.cmp = op, tuple(args), cmp

    def __and__(self, o): return SymBool("and", (self, SymBool.lift(o)))
    __rand__ = __and__
    def __or__(self, o): return SymBool("or", (self, SymBool.lift(o)))
    __ror__ = __or__
    def __invert__(self): return SymBool("not", (self,))

    @staticmethod
    def lift(v):
        if isinstance(v, SymBool):
            return v
        if isinstance(v, (bool, np.bool_)):
            return SymBool("const", (), bool(v))
        raise TraceError("cannot combine %r with a traced condition" % (v,))

    def __bool__(self):
        raise TraceError("a traced condition was used in `if` / `and` / `or` / `not`: combine comparisons with & | ~ instead "
                         "(the trace sees one symbolic evaluation, not one per chain)")


class SymComplex:
    """A complex parameter or intermediate as a pair of real nodes; complex arithmetic reduces to real arithmetic."""
    __array_priority__ = 1001.0
    __slots__ = ("re", "im")

    def __init__(self, re, im):
        self.re, self.im = Sym.lift(re), Sym.lift(im)

    @staticmethod
    def lift(v):
        if isinstance(v, SymComplex):
            return v
        if isinstance(v, Sym):
            return SymComplex(v, 0.0)
        if isinstance(v, (int, float, complex, np.number)) and not isinstance(v, (bool, np.bool_)):
            c = complex(v)
            return SymComplex(c.real, c.imag)
        raise TraceError("cannot use %r (%s) in a traced energy" % (v, type(v).__name__))

    def _bin(self, op, other, swap=False):
        if isinstance(other, np.ndarray):
            return NotImplemented
        a, b = (SymComplex.lift(other), self) if swap else (self, SymComplex.lift(other))
        if op == "add":
            return SymComplex(a.re + b.re, a.im + b.im)
        if op == "sub":
            return SymComplex(a.re - b.re, a.im - b.im)
        if op == "mul":
            return SymComplex(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re)
        if op == "div":
            den = b.re * b.re + b.im * b.im
            return SymComplex((a.re * b.re + a.im * b.im) / den, (a.im * b.re - a.re * b.im) / den)
        raise TraceError("unsupported complex operation %s" % op)

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("div", o)
    def __rtruediv__(self, o): return self._bin("div", o, True)
    def __neg__(self): return SymComplex(-self.re, -self.im)
    def __pos__(self): return self
    def __abs__(self): return Sym("sqrt", (self.re * self.re + self.im * self.im,))

    def __pow__(self, o):
        if isinstance(o, (int, np.integer)) or (isinstance(o, (float, np.floating)) and float(o).is_integer() and abs(o) <= 64):
            n = int(o)
            if n == 0:
                return SymComplex(1.0, 0.0)
            out, base, k = None, self, abs(n)
            while k:
                if k & 1:
                    out = base if out is None else out * base
                k >>= 1
                if k:
                    base = base * base
            return out if n > 0 else 1.0 / out
        raise TraceError("only integer powers of complex values can be traced")

    def conjugate(self): return SymComplex(self.re, -self.im)
    conj = conjugate
    real = property(lambda self: self.re)
    imag = property(lambda self: self.im)
    def absolute(self): return abs(self)
    def square(self): return self * self

    def __bool__(self):
        raise TraceError("the energy branches on a parameter value; a traced energy must be one arithmetic expression")

    def __complex__(self):
        raise TraceError("the energy converts a parameter to a Python complex (cmath.* functions): use numpy functions")
    __float__ = __complex__


def _real_part(v):
    if isinstance(v, SymComplex):
        return v.re
    if isinstance(v, (Sym, int, float, complex, np.number)) and not isinstance(v, (bool, np.bool_)):
        return v.real
    raise TraceError("cannot take the real part of %r in a traced energy" % (v,))


def _imag_part(v):
    if isinstance(v, SymComplex):
        return v.im
    if isinstance(v, (Sym, int, float, complex, np.number)) and not isinstance(v, (bool, np.bool_)):
        return v.imag
    raise TraceError("cannot take the imaginary part of %r in a traced energy" % (v,))


def _angle(v):
    return Sym.lift(_imag_part(v)).arctan2(_real_part(v))


class SymArray(np.ndarray):
    """The object arrays handed to a traced callable.  A plain object array answers ``.real`` with itself and ``.imag``
    with zeros, whatever its elements; here both act on each element (``SymComplex.re`` / ``.im``; a real :class:`Sym` is
    its own real part and has imaginary part 0), as on the reference's ``complex128`` arrays.  numpy keeps the subclass
    through ufuncs, so arrays computed from the parameters (``(c * c.conj()).real``, ``(c ** 2).imag``) behave the same;
    ``np.real`` / ``np.imag`` read these properties, ``np.conj`` calls each element's ``conjugate``, and ``np.angle``
    becomes ``arctan2(im, re)`` element by element.  Its priority is above the nodes', so that ``array * node`` is
    numpy's element-wise product rather than a deferral to the node."""
    __array_priority__ = 2000.0

    def _map(self, fn):
        out = np.empty(self.shape, dtype=object)
        for i, v in enumerate(self.flat):
            out.flat[i] = fn(v)
        return out.view(SymArray)

    real = property(lambda self: self._map(_real_part))
    imag = property(lambda self: self._map(_imag_part))

    def __array_wrap__(self, array, context=None, return_scalar=False):
        if array.ndim == 0:                           # a reduction (np.prod, ...): the node, as for a plain object array
            return array[()]
        return super().__array_wrap__(array, context, return_scalar)

    def __array_function__(self, func, types, args, kwargs):
        if func is np.angle:
            z = args[0] if args else kwargs["z"]
            deg = args[1] if len(args) > 1 else kwargs.get("deg", False)
            out = np.asanyarray(z).view(SymArray)._map(_angle)
            return out * (180.0 / math.pi) if deg else out
        return super().__array_function__(func, types, args, kwargs)


# --------------------------------------------------------------------------------------------------- tracing
def _inputs(n_real, n_complex):
    real = np.empty(n_real, dtype=object)
    for i in range(n_real):
        real[i] = Sym("x", value=i)
    cplx = np.empty(n_complex, dtype=object)
    for j in range(n_complex):
        cplx[j] = SymComplex(Sym("x", value=n_real + j), Sym("x", value=n_real + n_complex + j))
    return real.view(SymArray), cplx.view(SymArray)


def _scalar(v):
    if isinstance(v, np.ndarray):
        if v.size != 1:
            raise TraceError("the energy must return one number, got an array of shape %s" % (v.shape,))
        v = v.reshape(-1)[0]
    return v


def _call(fn, n_real, n_complex, what):
    """``fn`` on symbolic parameters; any failure is a :class:`TraceError` that names the original exception."""
    real, cplx = _inputs(n_real, n_complex)
    try:
        return _scalar(fn(real, cplx))
    except TraceError:
        raise
    except Exception as exc:
        raise TraceError("the %s cannot be traced: %s: %s" % (what, type(exc).__name__, exc)) from exc


def trace_energy(fn, n_real, n_complex):
    """Run ``fn(real_params, complex_params)`` on symbolic parameters; returns the real :class:`Sym` it computes (the real
    part of a complex-typed result, SURVEY.md quirk Q11: the Landau toy returns ``complex128`` with zero imaginary part)."""
    out = _call(fn, n_real, n_complex, "energy")
    if isinstance(out, SymComplex):
        out = out.re
    return Sym.lift(out)


def trace_reject(fn, n_real, n_complex):
    return SymBool.lift(_call(fn, n_real, n_complex, "reject condition"))


# --------------------------------------------------------------------------------------------------- numeric self-check
# d/da of the unary ops, for the rounding scale below
_DERIV = {"neg": lambda a, v: 1.0, "abs": lambda a, v: 1.0, "sqrt": lambda a, v: 0.5 / v, "exp": lambda a, v: v,
          "log": lambda a, v: 1.0 / a, "sin": lambda a, v: np.cos(a), "cos": lambda a, v: np.sin(a),
          "tan": lambda a, v: 1.0 + v * v, "tanh": lambda a, v: 1.0 - v * v, "sinh": lambda a, v: np.cosh(a),
          "cosh": lambda a, v: np.sinh(a), "arctan": lambda a, v: 1.0 / (1.0 + a * a)}
_FLOAT_OPS = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "neg": np.negative,
              "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "tan": np.tan,
              "tanh": np.tanh, "sinh": np.sinh, "cosh": np.cosh, "arctan": np.arctan, "arctan2": np.arctan2}
_FLOAT_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}


def _evaluate(root, x):
    """``(value, scale)`` of a recorded graph at the float64 state ``x``: the value, and a first-order bound on how far
    rounding can move it (in units of the unit roundoff: sums add the operands' scales, every other op weights them by its
    partial derivatives and adds its own result).  Comparisons evaluate to booleans with scale 0."""
    memo = {}
    stack = [(root, False)]
    while stack:
        node, ready = stack.pop()
        if id(node) in memo:
            continue
        if not ready and node.args:
            stack.append((node, True))
            stack.extend((a, False) for a in node.args)
            continue
        args = [memo[id(a)] for a in node.args]
        if isinstance(node, SymBool):
            if node.op == "cmp":
                v = bool(_FLOAT_CMP[node.cmp](args[0][0], args[1][0]))
            elif node.op == "const":
                v = bool(node.cmp)
            elif node.op == "not":
                v = not args[0][0]
            else:
                v = (args[0][0] and args[1][0]) if node.op == "and" else (args[0][0] or args[1][0])
            memo[id(node)] = (v, 0.0)
            continue
        if node.op == "x":
            v = np.float64(x[node.value])
            memo[id(node)] = (v, abs(v))
            continue
        if node.op == "const":
            memo[id(node)] = (np.float64(node.value), abs(node.value))
            continue
        v = _FLOAT_OPS[node.op](*[a[0] for a in args])
        if node.op in ("add", "sub"):
            s = args[0][1] + args[1][1]
        elif node.op == "mul":
            (a, sa), (b, sb) = args
            s = sa * abs(b) + abs(a) * sb
        elif node.op == "div":
            (a, sa), (b, sb) = args
            s = sa / abs(b) + abs(a) * sb / (b * b) + abs(v)
        elif node.op == "pow":
            (a, sa), (b, sb) = args
            s = abs(b * a ** (b - 1.0)) * sa + (abs(v * np.log(abs(a))) * sb if sb and v else 0.0) + abs(v)
        elif node.op == "arctan2":
            (a, sa), (b, sb) = args
            s = (abs(b) * sa + abs(a) * sb) / (a * a + b * b) + abs(v)
        else:
            a, sa = args[0]
            s = (abs(_DERIV[node.op](a, v)) * sa if sa else 0.0) + abs(v)
        memo[id(node)] = (v, s)
    return memo[id(root)]


def _numeric(fn, x, n_real, n_complex):
    out = _scalar(fn(x[:n_real].copy(), x[n_real:n_real + n_complex] + 1j * x[n_real + n_complex:]))
    return out if isinstance(out, (bool, np.bool_)) else complex(out).real


def _agree(got, want, scale):
    if isinstance(want, (bool, np.bool_)):
        return bool(got) == bool(want)
    if math.isnan(want):
        return True                                    # out of the callable's domain
    if math.isnan(got):
        return False
    if not math.isfinite(scale):
        return True                                    # no usable bound
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= 1e-8 * scale             # rounding is ~1e-16 * scale: a traced idiom gone wrong is not


def _self_check(node, fns, n_real, n_complex, states, what):
    """Compare the recorded graph with every callable in ``fns`` at ``states``; a disagreement is a TraceError."""
    with np.errstate(all="ignore"):
        for x in states:
            got, scale = _evaluate(node, x)
            for group, fn in fns:
                try:
                    want = _numeric(fn, x, n_real, n_complex)
                except Exception as exc:
                    raise TraceError("the %s fails on numbers: %s: %s" % (what, type(exc).__name__, exc)) from exc
                if not _agree(got, want, float(scale)):
                    raise TraceError(
                        "the traced %s%s computes %r where the function gives %r at real_params=%s, complex_params=%s: it "
                        "uses an operation that the trace records differently from numpy" % (
                            what, " (group %r)" % group if group else "", got, want, x[:n_real].tolist(),
                            (x[n_real:n_real + n_complex] + 1j * x[n_real + n_complex:]).tolist()))


def check_states(n_real, n_complex, initial=None):
    """The states of the self-check: 8 fixed-seed standard-normal states, then ``initial`` ([real | Re z | Im z]) if
    given."""
    states = list(np.random.default_rng(20261016).standard_normal((8, n_real + 2 * n_complex)))
    if initial is not None:
        states.append(np.asarray(initial, dtype=np.float64).reshape(-1))
    return states


# --------------------------------------------------------------------------------------------------- code generation
class _Emitter:
    """Straight-line C++ for a set of root nodes: every distinct (op, operands) is one ``const R tK``; ``a * b + c`` is
    written as one explicit fused multiply-add so that the value does not depend on which kernel the function is inlined in."""

    def __init__(self):
        self.lines, self.by_id, self.by_key, self.uses = [], {}, {}, {}

    @staticmethod
    def _leaf(n):
        return isinstance(n, Sym) and n.op in ("x", "const")

    def count(self, root):
        """How many times each node is used as an operand (a product used once may be folded into an fma)."""
        seen, stack = set(), [root]
        while stack:
            n = stack.pop()
            if id(n) in seen:
                continue
            seen.add(id(n))
            for a in n.args:
                self.uses[id(a)] = self.uses.get(id(a), 0) + 1
                stack.append(a)

    def operand(self, n):
        if isinstance(n, Sym) and n.op == "const":
            if math.isnan(n.value) or math.isinf(n.value):
                raise TraceError("the traced energy contains a non-finite constant")
            return "R(%s)" % repr(float(n.value))
        if isinstance(n, Sym) and n.op == "x":
            return "x[%d]" % n.value
        return self.by_id[id(n)]

    def emit(self, root):
        """Statements for everything ``root`` needs (iterative post-order: long sums are deep graphs); returns its name."""
        stack = [(root, False)]
        while stack:
            node, ready = stack.pop()
            if self._leaf(node) or id(node) in self.by_id:
                continue
            if not ready:
                stack.append((node, True))
                stack.extend((a, False) for a in node.args)
                continue
            args = [self.operand(a) for a in node.args]
            key = (type(node).__name__, node.op, getattr(node, "cmp", None)) + tuple(args)
            if key not in self.by_key:
                name = "%s%d" % ("b" if isinstance(node, SymBool) else "t", len(self.lines))
                self.lines.append(self._statement(node, name, args))
                self.by_key[key] = name
            self.by_id[id(node)] = self.by_key[key]
        return self.operand(root)

    def _statement(self, node, name, args):
        if isinstance(node, SymBool):
            if node.op == "cmp":
                expr = "(%s %s %s)" % (args[0], _COMPARE[node.cmp], args[1])
            elif node.op == "const":
                expr = "true" if node.cmp else "false"
            elif node.op == "not":
                expr = "(!%s)" % args[0]
            else:
                expr = "(%s %s %s)" % (args[0], "&&" if node.op == "and" else "||", args[1])
            return "const bool %s = %s;" % (name, expr)
        if node.op in ("add", "sub"):
            # a sum with a product in it: one explicit fma (the compiler would fuse one of the products anyway -- which one
            # may depend on the surrounding kernel)
            a, b = node.args
            if isinstance(b, Sym) and b.op == "mul" and self.uses.get(id(b), 0) <= 1:
                p, q = (self.operand(v) for v in b.args)
                return "const R %s = me_fma(%s%s, %s, %s);" % (name, "" if node.op == "add" else "-", p, q, args[0])
            if node.op == "add" and isinstance(a, Sym) and a.op == "mul" and self.uses.get(id(a), 0) <= 1:
                p, q = (self.operand(v) for v in a.args)
                return "const R %s = me_fma(%s, %s, %s);" % (name, p, q, args[1])
        template = _UNARY.get(node.op) or _BINARY.get(node.op)
        if template is None:
            raise TraceError("unsupported operation %s" % node.op)
        return "const R %s = %s;" % (name, template.format(*args))


_PRELUDE = '''// GENERATED by metropolisengine_amd.pyenergy from a Python energy callable -- do not edit.
#include "metropolis_user_energy.h"
__device__ __forceinline__ float me_py_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double me_py_abs(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float me_py_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double me_py_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float me_py_exp(float v) { return expf(v); }
__device__ __forceinline__ double me_py_exp(double v) { return exp(v); }
__device__ __forceinline__ float me_py_log(float v) { return logf(v); }
__device__ __forceinline__ double me_py_log(double v) { return log(v); }
__device__ __forceinline__ float me_py_sin(float v) { return sinf(v); }
__device__ __forceinline__ double me_py_sin(double v) { return sin(v); }
__device__ __forceinline__ float me_py_cos(float v) { return cosf(v); }
__device__ __forceinline__ double me_py_cos(double v) { return cos(v); }
__device__ __forceinline__ float me_py_tan(float v) { return tanf(v); }
__device__ __forceinline__ double me_py_tan(double v) { return tan(v); }
__device__ __forceinline__ float me_py_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ double me_py_tanh(double v) { return tanh(v); }
__device__ __forceinline__ float me_py_sinh(float v) { return sinhf(v); }
__device__ __forceinline__ double me_py_sinh(double v) { return sinh(v); }
__device__ __forceinline__ float me_py_cosh(float v) { return coshf(v); }
__device__ __forceinline__ double me_py_cosh(double v) { return cosh(v); }
__device__ __forceinline__ float me_py_atan(float v) { return atanf(v); }
__device__ __forceinline__ double me_py_atan(double v) { return atan(v); }
__device__ __forceinline__ float me_py_atan2(float a, float b) { return atan2f(a, b); }
__device__ __forceinline__ double me_py_atan2(double a, double b) { return atan2(a, b); }
__device__ __forceinline__ float me_py_pow(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double me_py_pow(double a, double b) { return pow(a, b); }
'''


def _function(header, roots, ret):
    """One device function: the statements of all roots (shared subexpressions once), then ``ret(names)``."""
    em = _Emitter()
    for r in roots:
        em.count(r)
    names = [em.emit(r) for r in roots]
    body = "".join("  %s\n" % line for line in em.lines)
    return "%s {\n%s%s}\n" % (header, body, ret(names))


def generate_source(energy, n_real, n_complex, reject=None, initial=None):
    """HIP source of the plugin for ``energy`` (a callable, or the reference's dictionary ``{"complex": {term: fn},
    "real": {...}, "all": {...}}``, metropolis_engine.py:111-116) and an optional ``reject`` callable.  Every traced graph
    is checked against its callable(s) at :func:`check_states` (``initial``: the engine's initial state, if known).
    Returns ``(source_text, term_names)``."""
    states = check_states(n_real, n_complex, initial)
    parts = [_PRELUDE]
    if isinstance(energy, dict):
        names = sorted(set().union(*[set(group) for group in energy.values()]))
        roots, groups = [], []
        for name in names:
            fns = [(group, energy[group][name]) for group in ("all", "real", "complex") if name in energy.get(group, {})]
            # one graph per name, traced from the first group that has it; every group's callable must compute it
            roots.append(trace_energy(fns[0][1], n_real, n_complex))
            distinct = list({id(fn): (group, fn) for group, fn in reversed(fns)}.values())
            _self_check(roots[-1], distinct if len(distinct) > 1 else [(None, fns[0][1])], n_real, n_complex, states,
                        "energy term %r" % name)
            groups.append((1 if name in energy.get("real", {}) else 0) | (2 if name in energy.get("complex", {}) else 0))
        parts.append("#define ME_USER_N_TERMS %d\n" % len(names))
        parts.append("constexpr unsigned me_user_term_groups(int term) { return %s; }\n" % " : ".join(
            ["term == %d ? %du" % (t, g) for t, g in enumerate(groups[:-1])] + ["%du" % groups[-1]]))
        cases = []
        for t, root in enumerate(roots):
            cases.append(_function("  if (term == %d)" % t, [root], lambda n: "    return %s;\n  " % n[0]))
        parts.append("template <typename R>\n__device__ R me_user_energy_term(int term, const R *x, const R *coef) {\n%s  return R(0);\n}\n"
                     % "".join(cases))
        term_names = tuple(names)
    else:
        root = trace_energy(energy, n_real, n_complex)
        _self_check(root, [(None, energy)], n_real, n_complex, states, "energy")
        parts.append(_function("template <typename R>\n__device__ R me_user_energy(const R *x, const R *coef)", [root],
                               lambda n: "  return %s;\n" % n[0]))
        term_names = ("total",)
    if reject is not None:
        cond = trace_reject(reject, n_real, n_complex)
        _self_check(cond, [(None, reject)], n_real, n_complex, states, "reject condition")
        parts.append("#define ME_USER_HAS_REJECT\n")
        parts.append(_function("template <typename R>\n__device__ bool me_user_reject(const R *x, const R *coef)", [cond],
                               lambda n: "  return %s;\n" % n[0]))
    return "".join(parts), term_names


class PythonEnergy(EnergySpec):
    """``energy_functions`` given as the reference gives it -- a Python callable ``(real_params, complex_params) -> float`` or
    its term dictionary -- traced at construction and compiled as a user plugin (see the module docstring).  ``reject`` is
    the reference's ``reject_condition`` callable (honoured when passed to the constructor; the reference drops it there,
    quirk Q6).  ``initial`` ([real | Re z | Im z]), if given, is one more state of the numeric self-check."""
    kind = _capi.ENERGY_USER

    def __init__(self, energy, reject=None, initial=None):
        if not (callable(energy) or isinstance(energy, dict)):
            raise TypeError("energy must be a callable or a dictionary of term callables")
        self.energy, self.reject, self.initial = energy, reject, initial
        self.term_names = tuple(sorted(set().union(*[set(g) for g in energy.values()]))) if isinstance(energy, dict) else ("total",)
        self.name = None
        self._loaded = set()

    def coefficients(self, n_real, n_complex):
        return np.zeros(0)                               # constants are literals of the generated source

    def build_plugin(self, n_real, n_complex):
        """Trace, write the generated source to ``_build/pyenergy/py<digest>.h`` and compile it (hipcc, once per distinct
        energy and dimensions; up to date plugins are reused).  Returns the plugin path; sets ``self.name``."""
        from . import build
        initial = self.initial if self.initial is not None and np.size(self.initial) == n_real + 2 * n_complex else None
        source, _ = generate_source(self.energy, n_real, n_complex, self.reject, initial)
        digest = hashlib.sha256(("%d,%d\n" % (n_real, n_complex) + source).encode()).hexdigest()[:16]
        self.name = "py" + digest
        directory = os.path.join(build.OBJ_DIR, "pyenergy")
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, self.name + ".h")
        if not os.path.exists(path) or open(path).read() != source:
            with open(path, "w") as fh:
                fh.write(source)
        return build.build_user_energy(path, self.name, n_real, n_complex)

    def ensure_loaded(self, n_real, n_complex):
        if (n_real, n_complex) in self._loaded:
            return
        plugin = self.build_plugin(n_real, n_complex)
        _capi.check(_capi.load().me_load_plugin(plugin.encode()))
        self._loaded.add((n_real, n_complex))


class PythonReject(RejectSpec):
    """The traced ``reject_condition`` of a :class:`PythonEnergy` plugin (``ME_REJECT_USER``)."""
    kind = _capi.REJECT_USER
