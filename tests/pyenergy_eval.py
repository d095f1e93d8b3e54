"""An interpreter of the expression graphs that metropolisengine_amd/pyenergy.py records (test infrastructure only): the
reference the traced energies are measured against.  Shared by tests/test_pyenergy_cpu.py, tests/test_pyenergy_corpus_cpu.py
and tests/test_gpu_pyenergy_corpus.py.

``x`` is one state ``[real | Re z | Im z]`` or a batch ``[n, D]``; the graph is evaluated in ``x``'s dtype (float64, or
``np.longdouble`` for a reference a few bits wider than the device's float64)."""
import numpy as np

from metropolisengine_amd import pyenergy as pe

_OPS = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "neg": np.negative,
        "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "tan": np.tan,
        "tanh": np.tanh, "sinh": np.sinh, "cosh": np.cosh, "arctan": np.arctan, "arctan2": np.arctan2}
_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}

# |d op / d a| for the unary ops, given the operand a and the value v
_SLOPE = {"neg": lambda a, v: 1, "abs": lambda a, v: 1, "sqrt": lambda a, v: 0.5 / v, "exp": lambda a, v: v,
          "log": lambda a, v: 1 / a, "sin": lambda a, v: np.cos(a), "cos": lambda a, v: np.sin(a),
          "tan": lambda a, v: 1 + v * v, "tanh": lambda a, v: 1 - v * v, "sinh": lambda a, v: np.cosh(a),
          "cosh": lambda a, v: np.sinh(a), "arctan": lambda a, v: 1 / (1 + a * a)}


def _walk(root, x, with_scale):
    """Post-order over the graph, each shared node once (traced graphs share subexpressions heavily, and long sums are
    deeper than Python's recursion limit)."""
    x = np.asarray(x)
    memo, stack = {}, [(root, False)]
    while stack:
        node, ready = stack.pop()
        if id(node) in memo:
            continue
        if not ready and node.args:
            stack.append((node, True))
            stack.extend((a, False) for a in node.args)
            continue
        memo[id(node)] = _node(node, [memo[id(a)] for a in node.args], x, with_scale)
    return memo[id(root)]


def _node(node, args, x, with_scale):
    if isinstance(node, pe.SymBool):
        if node.op == "cmp":
            v = _CMP[node.cmp](args[0][0], args[1][0])
        elif node.op == "const":
            v = np.bool_(node.cmp)
        elif node.op == "not":
            v = np.logical_not(args[0][0])
        else:
            v = (np.logical_and if node.op == "and" else np.logical_or)(args[0][0], args[1][0])
        return v, None
    if node.op == "x":
        v = x[..., node.value]
        return v, (np.abs(v) if with_scale else None)
    if node.op == "const":
        v = np.asarray(node.value, dtype=x.dtype)[()]
        return v, (np.abs(v) if with_scale else None)
    v = _OPS[node.op](*[a[0] for a in args])
    if not with_scale:
        return v, None
    # A: how far rounding in the operands and in this op can move v, in units of the unit roundoff (first order)
    if node.op in ("add", "sub"):
        s = args[0][1] + args[1][1]
    elif node.op == "mul":
        (a, sa), (b, sb) = args
        s = sa * np.abs(b) + np.abs(a) * sb
    elif node.op == "div":
        (a, sa), (b, sb) = args
        s = sa / np.abs(b) + np.abs(a) * sb / (b * b) + np.abs(v)
    elif node.op == "pow":
        (a, sa), (b, sb) = args
        s = np.abs(b * a ** (b - 1)) * sa + np.where((sb == 0) | (v == 0), 0, np.abs(v * np.log(np.abs(a))) * sb) + np.abs(v)
    elif node.op == "arctan2":
        (a, sa), (b, sb) = args
        # at (0, 0) the angle is exact if both zeros are, and unbounded if either is a rounded result
        den = a * a + b * b
        s = np.where(sa + sb == 0, 0, np.where(den == 0, np.inf, (np.abs(b) * sa + np.abs(a) * sb) / den)) + np.abs(v)
    else:
        a, sa = args[0]
        s = np.where(sa == 0, 0, np.abs(_SLOPE[node.op](a, v)) * sa) + np.abs(v)
    return v, s


def evaluate(node, x):
    """The value of a recorded :class:`~metropolisengine_amd.pyenergy.Sym` / ``SymBool`` graph at ``x``."""
    with np.errstate(all="ignore"):
        return _walk(node, x, False)[0]


def evaluate_scaled(node, x):
    """``(value, A)``: the value, and the rounding scale ``A >= 0`` of the graph at ``x`` -- sums add their operands'
    scales (the cancellation scale: ``|a| + |b|`` for leaves), every other op weights them by the magnitude of its
    partial derivatives and adds its own result.  Computing the graph in a precision with unit roundoff ``eps`` lands
    within a small multiple of ``eps * A`` of the exact value (plus underflow)."""
    with np.errstate(all="ignore"):
        return _walk(node, x, True)


def comparison_margin(node, x):
    """The smallest ``|a - b| / (A_a + A_b)`` over the comparisons of a traced condition at ``x`` (batch: per row): a
    boolean that a rounding error could flip has a margin near 0."""
    margin = np.full(np.asarray(x).shape[:-1], np.inf)
    seen, stack = set(), [node]
    with np.errstate(all="ignore"):
        while stack:
            n = stack.pop()
            if id(n) in seen or not isinstance(n, pe.SymBool):
                continue
            seen.add(id(n))
            if n.op == "cmp":
                (a, sa), (b, sb) = (_walk(arg, x, True) for arg in n.args)
                margin = np.minimum(margin, np.nan_to_num(np.abs(a - b) / (sa + sb), nan=np.inf))
            stack.extend(n.args)
    return margin


def error_ratio(got, ref, scale, dtype):
    """``|got - ref| / (eps * A + tiny)`` element by element, ``eps`` / ``tiny`` of ``dtype`` (the machine epsilon and the
    smallest normal number: underflow to zero or a subnormal is within ``tiny``).  0 where both are NaN or the same
    infinity; inf where only one is NaN, or an infinity meets anything else."""
    fi = np.finfo(dtype)
    got, ref, scale = (np.asarray(v, dtype=np.longdouble) for v in (got, ref, scale))
    with np.errstate(all="ignore"):
        ratio = np.abs(got - ref) / (np.longdouble(fi.eps) * scale + np.longdouble(fi.tiny))
    both_nan = np.isnan(got) & np.isnan(ref)
    same_inf = np.isinf(got) & (got == ref)
    ratio = np.where(both_nan | same_inf, 0, ratio)
    return np.where(np.isnan(ratio), np.inf, ratio)
