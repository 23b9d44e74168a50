"""First-play urgency (Engine.set_fpu, include/azx.h) above the engine: one normaliser and one `apply`.

FPU is a property of an engine's SEARCH, not a self-play option: it is not in selfplay_options.OPTIONS, matches and
tournaments take engines that have it set, and every layer that builds an engine for a Policy -- Policy itself (the
single-game path), Player (device self-play, external_batch, both engines of device_match) and evaluation
(evaluate_throughput's pairs and tournaments) -- puts the policy's `fpu` on it.  A Policy gets it from config["fpu"]
(Policy.initialize), Policy.set_fpu or Player(fpu=...).  NOT the reference's behaviour; off by default; outside every
parity claim.
"""
import numpy as np

MODES = ("absolute", "reduction")
DEFAULT = ("reduction", 0.0, 0.25, 0.0)


def _number(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("fpu: %s must be a number, got %r" % (name, v))
    return float(v)


def normalize_fpu(fpu):
    """(mode, value, reduction, root_reduction) of True (= the default, ("reduction", 0.0, 0.25, 0.0)), "absolute" /
    "reduction" (the rest default), a 4-tuple in that order or a mapping with the keys "mode", "value", "reduction",
    "root_reduction" (any subset: the rest default); None for off (None, False, "off", mode "off").  A ValueError unless
    mode is "absolute" or "reduction", value a number in [-1, 1] and the reductions finite numbers >= 0.  The defaults
    (reduction 0.25 below the root, 0 at it) are lc0's / KataGo's customary values as the author recalls them and are not
    checked here."""
    if fpu is None or fpu is False or (isinstance(fpu, str) and fpu == "off"):
        return None
    mode, value, red, root_red = DEFAULT
    if fpu is True:
        pass
    elif isinstance(fpu, str):
        mode = fpu
    elif isinstance(fpu, dict):
        extra = set(fpu) - {"mode", "value", "reduction", "root_reduction"}
        if extra:
            raise ValueError("fpu as a dict takes the keys 'mode', 'value', 'reduction' and 'root_reduction', got %r"
                             % (sorted(map(str, fpu)),))
        mode, value = fpu.get("mode", mode), fpu.get("value", value)
        red, root_red = fpu.get("reduction", red), fpu.get("root_reduction", root_red)
    elif isinstance(fpu, (tuple, list)) and len(fpu) == 4:
        mode, value, red, root_red = fpu
    else:
        raise ValueError("fpu must be True, 'absolute', 'reduction', a (mode, value, reduction, root_reduction) tuple or "
                         "a dict with those keys, got %r" % (fpu,))
    if mode == "off":
        return None
    if mode not in MODES:
        raise ValueError("fpu: mode must be 'off', 'absolute' or 'reduction', got %r" % (mode,))
    value, red, root_red = _number("value", value), _number("reduction", red), _number("root_reduction", root_red)
    if not -1.0 <= value <= 1.0:                    # NaN fails both comparisons
        raise ValueError("fpu: value must be in [-1, 1], got %r" % (value,))
    for name, v in (("reduction", red), ("root_reduction", root_red)):
        if not 0.0 <= v < float("inf"):
            raise ValueError("fpu: %s must be finite and >= 0, got %r" % (name, v))
    return mode, value, red, root_red


def policy_fpu(policy):
    """The normalised setting a Policy carries (None: off; duck-typed policies without the attribute: off)."""
    return normalize_fpu(getattr(policy, "fpu", None))


def apply(engine, fpu):
    """Put the normalised `fpu` (None: off) on `engine` unless it is what the engine already has: Engine.set_fpu zeroes
    fpu_stats(), so an unchanged setting is left alone."""
    want = ("off", 0.0, 0.0, 0.0) if fpu is None else tuple(fpu)
    if getattr(engine, "_fpu_applied", ("off", 0.0, 0.0, 0.0)) == want:
        return
    if fpu is None:
        engine.clear_fpu()
    else:
        engine.set_fpu(*want)
    engine._fpu_applied = want
