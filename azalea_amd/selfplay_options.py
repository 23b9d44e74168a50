"""The opt-in rules of throughput self-play, as one table: what Player, policy_trainer.train and the Engine each need
to know of an option stands once, in its entry of OPTIONS, in the order the options are applied to an engine.  None of
them is the reference's behaviour; all are off by default (DESIGN 7.9-7.15 have the rules, 7.17 this table).

Adding an option: its normaliser and its entry here, its keyword and docstring paragraph in Player.__init__, its
paragraph in train's docstring, and Engine's set_* / *_stats pair.  Player's checks and stats, the engine set-up and
train's config handling and log lines follow from the entry.
"""
import numpy as np

from . import engine as _eng


def normalize_playout_cap(cap):
    """(full_prob, fast_simulations) of a pair or of a {"full_prob": ..., "fast_simulations": ...} mapping; a
    ValueError unless full_prob is in (0, 1] and fast_simulations a whole number >= 1."""
    try:
        if isinstance(cap, dict):
            if set(cap) != {"full_prob", "fast_simulations"}:
                raise ValueError
            full_prob, fast = cap["full_prob"], cap["fast_simulations"]
        else:
            full_prob, fast = cap
        full_prob = float(full_prob)
        if isinstance(fast, bool) or int(fast) != fast:
            raise ValueError
        fast = int(fast)
    except (TypeError, ValueError, KeyError):
        raise ValueError("playout_cap must be (full_prob, fast_simulations) or a dict with exactly these two keys, "
                         "got %r" % (cap,)) from None
    if not 0.0 < full_prob <= 1.0:
        raise ValueError("playout_cap: full_prob %r outside (0, 1]" % full_prob)
    if fast < 1:
        raise ValueError("playout_cap: fast_simulations %d below 1" % fast)
    return full_prob, fast


def normalize_selfplay_openings(spec, board_size=None):
    """(book, weights) of a self-play opening book -- book a list of move lists (tile + 1 in play order), weights a list
    of floats or None for uniform -- or None for None.  Accepted: a list of move lists; {"book": [...]} with an optional
    "weights": [...]; {"all": 1 | 2} for engine.all_openings(board_size, plies) (needs `board_size`); and in a dict an
    optional "empty_share": s in [0, 1], which puts the empty opening first with weight s and gives the others 1 - s in
    equal parts (not together with "weights").  A ValueError for anything else: unknown keys, both or neither of "book"
    and "all", an empty book, moves that are not whole numbers, weights of another length, or negative, non-finite or
    all zero.  The rules themselves (moves on the board, no tile twice, undecided) are engine.openings_check's."""
    if spec is None:
        return None
    what = "selfplay_openings"
    weights, share = None, None
    if isinstance(spec, dict):
        extra = set(spec) - {"book", "weights", "all", "empty_share"}
        if extra:
            raise ValueError("%s as a dict takes the keys 'book', 'weights', 'all' and 'empty_share', got %r"
                             % (what, sorted(map(str, spec))))
        if ("book" in spec) == ("all" in spec):
            raise ValueError("%s as a dict needs exactly one of 'book' and 'all'" % what)
        if "all" in spec:
            plies = spec["all"]
            if isinstance(plies, bool) or plies not in (1, 2):
                raise ValueError("%s: 'all' must be 1 or 2 (plies), got %r" % (what, plies))
            if board_size is None:
                raise ValueError("%s: 'all' needs the board size" % what)
            book = _eng.all_openings(int(board_size), int(plies))
        else:
            book = spec["book"]
        weights, share = spec.get("weights"), spec.get("empty_share")
    else:
        book = spec
    try:
        if isinstance(book, (str, bytes, dict)):
            raise TypeError
        book = [list(o) for o in book]
        for o in book:
            for m in o:
                if isinstance(m, bool) or int(m) != m:
                    raise ValueError
        book = [[int(m) for m in o] for o in book]
    except (TypeError, ValueError):
        raise ValueError("%s: the book must be a list of move lists (whole numbers, tile + 1 in play order), got %r"
                         % (what, spec)) from None
    if not book:
        raise ValueError("%s: the book is empty (leave the option out to play from the empty board)" % what)
    if share is not None:
        if weights is not None:
            raise ValueError("%s: 'empty_share' and 'weights' cannot be given together" % what)
        if isinstance(share, bool) or not isinstance(share, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(share) <= 1.0:
            raise ValueError("%s: empty_share must be a number in [0, 1], got %r" % (what, share))
        share = float(share)
        weights = [share] + [(1.0 - share) / len(book)] * len(book)
        book = [[]] + book
    if weights is not None:
        try:
            if isinstance(weights, (str, bytes, dict)):
                raise TypeError
            weights = [float(w) for w in weights]
        except (TypeError, ValueError):
            raise ValueError("%s: weights must be a list of numbers, got %r" % (what, weights)) from None
        if len(weights) != len(book):
            raise ValueError("%s: %d weights for %d openings" % (what, len(weights), len(book)))
        if any(not np.isfinite(w) or w < 0.0 for w in weights):
            raise ValueError("%s: weights must be finite and >= 0, got %r" % (what, weights))
        if not sum(weights) > 0.0:
            raise ValueError("%s: the weights are all zero" % what)
    return book, weights


def normalize_train_targets(train_targets):
    """(policy_rows, value_mix) of "visits" (= ("visits", 0.0)), of a pair or of a {"policy_rows": ..., "value_mix": ...}
    mapping; None for None / False and for the pair that is "off", ("reference", 0.0).  A ValueError unless policy_rows
    is "reference" or "visits" and value_mix a number in [0, 1]."""
    if train_targets is None or train_targets is False:
        return None
    if isinstance(train_targets, str):
        if train_targets != "visits":
            raise ValueError("train_targets must be 'visits', a (policy_rows, value_mix) pair or a dict with those "
                             "keys, got %r" % (train_targets,))
        return "visits", 0.0
    if isinstance(train_targets, dict):
        if set(train_targets) != {"policy_rows", "value_mix"}:
            raise ValueError("train_targets as a dict needs exactly the keys 'policy_rows' and 'value_mix', got %r"
                             % (sorted(map(str, train_targets)),))
        rows, mix = train_targets["policy_rows"], train_targets["value_mix"]
    elif isinstance(train_targets, (tuple, list)) and len(train_targets) == 2:
        rows, mix = train_targets
    else:
        raise ValueError("train_targets must be 'visits', a (policy_rows, value_mix) pair or a dict with those keys, "
                         "got %r" % (train_targets,))
    if rows not in ("reference", "visits"):
        raise ValueError("train_targets: policy_rows must be 'reference' or 'visits', got %r" % (rows,))
    if isinstance(mix, (bool, np.bool_)) or not isinstance(mix, (int, float, np.integer, np.floating)):
        raise ValueError("train_targets: value_mix must be a number in [0, 1], got %r" % (mix,))
    mix = float(mix)
    if not 0.0 <= mix <= 1.0:                  # (NaN fails both comparisons)
        raise ValueError("train_targets: value_mix must be in [0, 1], got %r" % (mix,))
    if rows == "reference" and mix == 0.0:
        return None
    return rows, mix


def normalize_forced_playouts(forced_playouts):
    """(k, prune) of True (= (2.0, True)), a pair or a {"k": ..., "prune": ...} mapping, or None for off (None, False,
    (0, False)); a ValueError unless k is a number in [0, 64], prune a bool, and k > 0 where prune is set."""
    if forced_playouts is None or forced_playouts is False:
        return None
    if forced_playouts is True:
        return 2.0, True
    if isinstance(forced_playouts, dict):
        if set(forced_playouts) != {"k", "prune"}:
            raise ValueError("forced_playouts as a dict needs exactly the keys 'k' and 'prune', got %r"
                             % (sorted(map(str, forced_playouts)),))
        k, prune = forced_playouts["k"], forced_playouts["prune"]
    elif isinstance(forced_playouts, (tuple, list)) and len(forced_playouts) == 2:
        k, prune = forced_playouts
    else:
        raise ValueError("forced_playouts must be True, a (k, prune) pair or a dict with those keys, got %r"
                         % (forced_playouts,))
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise ValueError("forced_playouts: k must be a number in [0, 64], got %r" % (k,))
    k = float(k)
    if not 0.0 <= k <= 64.0:                        # NaN fails both comparisons
        raise ValueError("forced_playouts: k must be in [0, 64], got %r" % (k,))
    if not isinstance(prune, (bool, np.bool_)):
        raise ValueError("forced_playouts: prune must be True or False, got %r" % (prune,))
    if k == 0.0:
        if prune:
            raise ValueError("forced_playouts: pruning needs forcing (k > 0), got k = 0 with prune = True")
        return None
    return k, bool(prune)


GUMBEL_DEFAULT = (16, 50.0, 1.0, True)


def normalize_gumbel(gumbel):
    """(m, c_visit, c_scale, improved_rows) of True (= (16, 50.0, 1.0, True)), an int m, an (m, c_visit, c_scale)
    triple or a mapping with the keys "m", "c_visit", "c_scale", "improved_rows" (any subset: the rest default), or None
    for off (None, False, m = 0); a ValueError unless m is an int in [2, 64], c_visit a number in [0, 1e4], c_scale a
    number in (0, 100] and improved_rows a bool.  The defaults 50 and 1.0 are the author's recollection of the paper's
    board-game values and are not checked here."""
    if gumbel is None or gumbel is False:
        return None
    m, c_visit, c_scale, rows = GUMBEL_DEFAULT
    if gumbel is True:
        pass
    elif isinstance(gumbel, dict):
        extra = set(gumbel) - {"m", "c_visit", "c_scale", "improved_rows"}
        if extra:
            raise ValueError("gumbel as a dict takes the keys 'm', 'c_visit', 'c_scale' and 'improved_rows', got %r"
                             % (sorted(map(str, gumbel)),))
        m, c_visit = gumbel.get("m", m), gumbel.get("c_visit", c_visit)
        c_scale, rows = gumbel.get("c_scale", c_scale), gumbel.get("improved_rows", rows)
    elif isinstance(gumbel, (tuple, list)) and len(gumbel) == 3:
        m, c_visit, c_scale = gumbel
    elif isinstance(gumbel, (int, np.integer)):
        m = gumbel
    else:
        raise ValueError("gumbel must be True, an int m, an (m, c_visit, c_scale) triple or a dict with those keys, "
                         "got %r" % (gumbel,))
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
        raise ValueError("gumbel: m must be an int in [2, 64] (0 is off), got %r" % (m,))
    m = int(m)
    if m == 0:
        return None
    if not 2 <= m <= 64:
        raise ValueError("gumbel: m must be in [2, 64] (0 is off), got %r" % (m,))
    for name, v in (("c_visit", c_visit), ("c_scale", c_scale)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("gumbel: %s must be a number, got %r" % (name, v))
    c_visit, c_scale = float(c_visit), float(c_scale)
    if not 0.0 <= c_visit <= 1.0e4:                  # NaN fails both comparisons
        raise ValueError("gumbel: c_visit must be in [0, 1e4], got %r" % (c_visit,))
    if not 0.0 < c_scale <= 100.0:
        raise ValueError("gumbel: c_scale must be in (0, 100], got %r" % (c_scale,))
    if not isinstance(rows, (bool, np.bool_)):
        raise ValueError("gumbel: improved_rows must be True or False, got %r" % (rows,))
    return m, c_visit, c_scale, bool(rows)


def normalize_early_stop(early_stop):
    """`early_stop` as a bool; a ValueError for anything but True / False (None counts as False)."""
    if early_stop is None:
        return False
    if not isinstance(early_stop, (bool, np.bool_)):
        raise ValueError("early_stop must be True or False, got %r" % (early_stop,))
    return bool(early_stop)


def normalize_resign(resign):
    """(threshold, min_ply, keep_prob) of a triple or of a {"threshold": ..., "min_ply": ..., "keep_prob": ...}
    mapping; a ValueError unless threshold is in [-1, 1], min_ply a whole number >= 0 and keep_prob in [0, 1]."""
    try:
        if isinstance(resign, dict):
            if set(resign) != {"threshold", "min_ply", "keep_prob"}:
                raise ValueError
            thr, min_ply, keep = resign["threshold"], resign["min_ply"], resign["keep_prob"]
        else:
            thr, min_ply, keep = resign
        thr, keep = float(thr), float(keep)
        if isinstance(min_ply, bool) or int(min_ply) != min_ply:
            raise ValueError
        min_ply = int(min_ply)
    except (TypeError, ValueError, KeyError):
        raise ValueError("resign must be (threshold, min_ply, keep_prob) or a dict with exactly these three keys, "
                         "got %r" % (resign,)) from None
    if not -1.0 <= thr <= 1.0:              # (false for NaN)
        raise ValueError("resign: threshold %r outside [-1, 1]" % thr)
    if min_ply < 0:
        raise ValueError("resign: min_ply %d is negative" % min_ply)
    if not 0.0 <= keep <= 1.0:
        raise ValueError("resign: keep_prob %r outside [0, 1]" % keep)
    return thr, min_ply, keep


# ---- what is specific to one option, as the hook its entry names -------------------------------------------------
def _fast_simulations_fit(player, cap, pol):
    if cap[1] > pol.simulations:
        raise ValueError("playout_cap: fast_simulations %d above the policy's simulations %d" % (cap[1], pol.simulations))
    return cap


def _fast_simulations_fit_config(cap, config, policy):
    if cap[1] > policy.simulations:
        raise ValueError("config['playout_cap']: fast_simulations %d above simulations %d" % (cap[1], policy.simulations))
    return cap


def _book_given(openings, weights):
    """Player's selfplay_openings / selfplay_opening_weights before the mode is known: the pair, or None for off (the
    book is normalised by _book_for_board, once the agents have been looked at)."""
    if openings is None:
        if weights is not None:
            raise ValueError("selfplay_opening_weights given without selfplay_openings")
        return None
    return openings, weights


def _single_agent(player):
    if len(player.agents) != 1:
        raise ValueError("selfplay_openings is a self-play option: it needs a single agent, got %d (two agents play "
                         "through the host loop or, with device_match=True, a device match)" % len(player.agents))


def _book_for_board(player, given, pol):
    openings, weights = given
    n = player.agents[0].game.board_size
    book, w = normalize_selfplay_openings(openings, n)
    if weights is not None:
        if w is not None:
            raise ValueError("selfplay_openings: weights given twice (in the book's dict and as selfplay_opening_weights)")
        book, w = normalize_selfplay_openings({"book": book, "weights": weights}, n)
    _eng.openings_check(n, book)
    return book, w


class Option:
    """One self-play option.  `name` is the Player keyword and the config[...] key (`keywords`: all the Player keywords
    it is given through, in the order of a normalised value's parts, where there are several); `normalize` the
    normaliser of train (`config_args`: the further config keys it takes; `config_prefix`: train names the key in front
    of the normaliser's message; `config_check(value, config, policy)`: what train holds beyond it) and, unless `given`
    stands in for it there, of Player; `off` what both hold while the option is off; `match_reason` / `host_reason` the
    clauses of Player's two refusals; `requires(player)` / `fits(player, value, policy)` Player's checks before / after
    the host-loop refusal, `fits` returning the value to keep; `setter` / `stats` the names of Engine's setter (given the
    value, a tuple's parts as its arguments) and stats method; `excludes` the options it cannot be set beside, because
    of `excludes_reason`; `title` and `log(value)` the two halves of train's log line."""

    def __init__(self, name, normalize, match_reason, host_reason, setter, stats, title, log, off=None, keywords=None,
                 given=None, requires=None, fits=None, excludes=(), excludes_reason=None,
                 config_args=(), config_prefix=True, config_check=None):
        self.name, self.normalize, self.off = name, normalize, off
        self.keywords = keywords or (name,)
        self.match_reason, self.host_reason = match_reason, host_reason
        self.given, self.requires, self.fits = given, requires, fits
        self.setter, self.stats = setter, stats
        self.excludes, self.excludes_reason = tuple(excludes), excludes_reason
        self.title, self.log = title, log
        self.config_args, self.config_prefix, self.config_check = tuple(config_args), config_prefix, config_check

    def is_on(self, value):
        return value is not None and value is not False

    def apply(self, engine, value):
        """The normalised `value` onto `engine` (nothing while the option is off)."""
        if self.is_on(value):
            getattr(engine, self.setter)(*(value if isinstance(value, tuple) else (value,)))

    def excluded_by(self, value, others):
        """The first option of `excludes` that is on in `others` (name -> value) beside this one, or None."""
        if self.is_on(value):
            for other in self.excludes:
                if BY_NAME[other].is_on(others[other]):
                    return other
        return None

    def exclusion_text(self, other, config=False):
        if config:
            return "config['%s']: %s cannot be set together with config['%s']: %s" % (self.name, self.name, other,
                                                                                      self.excludes_reason)
        return "%s cannot be set together with %s: %s" % (self.name, other, self.excludes_reason)


# In the order Player applies them to a new engine (the book first: generation 0 follows it too).
OPTIONS = (
    Option("selfplay_openings", normalize_selfplay_openings,
           keywords=("selfplay_openings", "selfplay_opening_weights"), config_args=("board_size",),
           given=_book_given, requires=_single_agent, fits=_book_for_board,
           match_reason="a device match starts its games from its own book (use openings=; engine.Match refuses an "
                        "engine with a self-play book)",
           host_reason="starts every game from the empty board",
           setter="set_selfplay_openings", stats="selfplay_openings_stats", title="self-play opening book",
           log=lambda v: "every game starts from one of %d openings, %s, drawn on the device from its uid"
                         % (len(v[0]), "uniform" if v[1] is None else "weighted")),
    Option("playout_cap", normalize_playout_cap, fits=_fast_simulations_fit,
           config_prefix=False, config_check=_fast_simulations_fit_config,
           match_reason="a device match records one row per moved ply (engine.Match refuses an engine with a cap)",
           host_reason="searches every ply in full",
           setter="set_playout_cap", stats="playout_cap_stats", title="playout cap randomisation",
           log=lambda v: "a ply is a full search with probability %g, else %d simulations without noise and without a "
                         "training row" % v),
    Option("resign", normalize_resign, config_prefix=False,
           match_reason="a device match plays every game to the end (engine.Match refuses an engine with resignation set)",
           host_reason="plays every game to the end",
           setter="set_resign", stats="resign_stats", title="resignation",
           log=lambda v: "the mover resigns below a root value of %g from ply %d on; a share %g of the games is exempt "
                         "and measures the false positives" % v),
    Option("early_stop", normalize_early_stop, off=False,
           match_reason="a device match searches every ply in full (engine.Match refuses an engine with early stop set)",
           host_reason="runs every search to its last simulation",
           setter="set_early_stop", stats="early_stop_stats", title="early stop",
           log=lambda v: "a search drawn at temperature 0 stops once its leading root child cannot be caught"),
    Option("train_targets", normalize_train_targets,
           match_reason="a device match's harvest records the reference's rows and the outcome (engine.Match refuses an "
                        "engine with training targets set)",
           host_reason="records the reference's rows and the outcome",
           setter="set_train_targets", stats="train_targets_stats", title="training targets",
           log=lambda v: "policy rows '%s', reward (1 - %g) * z + %g * v" % (v[0], v[1], v[1])),
    Option("forced_playouts", normalize_forced_playouts,
           match_reason="a device match searches and draws every ply as the reference does (engine.Match refuses an "
                        "engine with forced playouts set)",
           host_reason="selects by PUCT alone and records every visit",
           setter="set_forced_playouts", stats="forced_playouts_stats", title="forced playouts",
           log=lambda v: "k = %g, policy target pruning %s" % (v[0], "on" if v[1] else "off")),
    Option("gumbel", normalize_gumbel,
           excludes=("forced_playouts", "early_stop"),
           excludes_reason="that option is a rule about PUCT visit leaders, which a Gumbel root search does not play",
           match_reason="a device match searches and draws every ply as the reference does (engine.Match refuses an "
                        "engine with the Gumbel root search set)",
           host_reason="selects by PUCT and draws from the visit counts",
           setter="set_gumbel", stats="gumbel_stats", title="Gumbel root search",
           log=lambda v: "m = %d, c_visit = %g, c_scale = %g, rows = %s"
                         % (v[0], v[1], v[2], "the improved policy" if v[3] else "from the visit counts")),
)
BY_NAME = {opt.name: opt for opt in OPTIONS}

# train() reads and reports them in this order: the book, then the others from the last applied to the first
TRAIN_ORDER = OPTIONS[:1] + OPTIONS[:0:-1]


def from_config(config, policy):
    """train()'s part: (Player keywords, log lines) of the self-play options in `config`, every key normalised -- a
    ValueError that names the key, before anything is built -- and every exclusion judged once both sides are known."""
    values, judged = {}, set()
    for opt in TRAIN_ORDER:
        raw = config.get(opt.name)
        try:
            value = opt.off if raw is None else opt.normalize(raw, *(config.get(k) for k in opt.config_args))
        except ValueError as exc:
            if not opt.config_prefix:
                raise
            raise ValueError("config['%s']: %s" % (opt.name, exc)) from None
        if opt.config_check is not None and opt.is_on(value):
            value = opt.config_check(value, config, policy)
        values[opt.name] = value
        for o in OPTIONS:
            if o.excludes and o.name not in judged and all(n in values for n in (o.name,) + o.excludes):
                judged.add(o.name)
                other = o.excluded_by(values[o.name], values)
                if other is not None:
                    raise ValueError(o.exclusion_text(other, config=True))
    keywords, lines = {}, []
    for opt in TRAIN_ORDER:
        value = values[opt.name]
        on = opt.is_on(value)
        parts = value if len(opt.keywords) > 1 and on else (value,) * len(opt.keywords)
        keywords.update(zip(opt.keywords, parts))
        lines.append("%s (config['%s']): %s" % (opt.title, opt.name, "on -- NOT the reference's behaviour: " + opt.log(value)
                                                 if on else "off"))
    return keywords, lines
