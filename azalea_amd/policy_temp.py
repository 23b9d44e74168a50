"""Policy temperature of the search's priors (Engine.set_policy_temp, include/azx.h) above the engine: one normaliser
and one `apply`.

Like first-play urgency (azalea_amd/fpu.py) it is a property of an engine's SEARCH, not a self-play option: it is not in
selfplay_options.OPTIONS, matches and tournaments take engines that have it set, and every layer that builds an engine
for a Policy -- Policy itself (the single-game path), Player (device self-play, external_batch, both engines of
device_match) and evaluation (evaluate_batched, evaluate_throughput's pairs and tournaments) -- puts the policy's
`policy_temp` on it.  A Policy gets it from config["policy_temp"] (Policy.initialize), Policy.set_policy_temp or
Player(policy_temp=...).  Checkpoints do not carry it.  NOT the reference's behaviour; off by default; outside every
parity claim.
"""
import numpy as np

OFF = (8, 8)


def _eighths(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("policy_temp: %s must be an integer in 1..8, got %r" % (name, v))
    v = int(v)
    if not 1 <= v <= 8:
        raise ValueError("policy_temp: %s must be in 1..8 (8 is off; the temperature is 8 / %s), got %r" % (name, name, v))
    return v


def normalize_policy_temp(policy_temp):
    """(eighths, root_eighths) of an int m (= (m, 8): the rows the search expands from at temperature 8 / m, the root
    select untouched), a 2-tuple / list in that order or a mapping with the keys "eighths" and "root_eighths" (either
    one: the other is 8); None for off (None, False, (8, 8), 8).  A ValueError unless both are integers in 1..8.
    True is refused: the option has no default setting."""
    if policy_temp is None or policy_temp is False:
        return None
    if policy_temp is True:
        raise ValueError("policy_temp has no default setting: give eighths (an int), (eighths, root_eighths) or a dict")
    if isinstance(policy_temp, dict):
        extra = set(policy_temp) - {"eighths", "root_eighths"}
        if extra:
            raise ValueError("policy_temp as a dict takes the keys 'eighths' and 'root_eighths', got %r"
                             % (sorted(map(str, policy_temp)),))
        m, r = policy_temp.get("eighths", 8), policy_temp.get("root_eighths", 8)
    elif isinstance(policy_temp, (tuple, list)):
        if len(policy_temp) != 2:
            raise ValueError("policy_temp as a tuple is (eighths, root_eighths), got %r" % (policy_temp,))
        m, r = policy_temp
    elif isinstance(policy_temp, (int, np.integer)):
        m, r = policy_temp, 8
    else:
        raise ValueError("policy_temp must be an int, an (eighths, root_eighths) tuple, a dict with those keys or None, "
                         "got %r" % (policy_temp,))
    m, r = _eighths("eighths", m), _eighths("root_eighths", r)
    return None if (m, r) == OFF else (m, r)


def policy_policy_temp(policy):
    """The normalised setting a Policy carries (None: off; duck-typed policies without the attribute: off)."""
    return normalize_policy_temp(getattr(policy, "policy_temp", None))


def apply(engine, policy_temp):
    """Put the normalised `policy_temp` (None: off) on `engine` unless it is what the engine already has:
    Engine.set_policy_temp zeroes policy_temp_stats(), so an unchanged setting is left alone."""
    want = OFF if policy_temp is None else tuple(policy_temp)
    if getattr(engine, "_policy_temp_applied", OFF) == want:
        return
    if policy_temp is None:
        engine.clear_policy_temp()
    else:
        engine.set_policy_temp(*want)
    engine._policy_temp_applied = want
