"""What to do with a single-launch update sweep that did not get through on one GPU.

The single-launch sweep needs all its workgroups resident at once.  If the GPU could not give it that (CUs held by another
stream or process: its in-kernel exchange times out; or the device cannot hold the grid at all), it is redone on HALF the
workgroups, each walking through twice the objectives (about twice the time: kh_set_update_workgroups), then on an eighth,
and only then interval by interval -- one launch each, nothing waits inside a kernel, ten times the time -- like the
sharded path does.  Anything else than a timeout / "cannot be resident" is a real error.

No torch, no GPU: of the engine only ``set_update_workgroups``, ``set_row_split`` and ``row_split`` are touched.
"""
import logging

from ._lib import KH_ERR_TIMEOUT, KH_ERR_UNSUPPORTED, KrotovHipError

_FULL_GRID_PROBE_EVERY = 16  # update sweeps in a row on a reduced grid before the full one is tried again


def leave_row_split(engine, what, exc):
    """A sweep (``what``: 'forward', 'backward', 'update') of an engine with ``row_split`` > 1 timed out -- its workgroups
    were not all resident --: one workgroup per objective from here on; the caller redoes the sweep."""
    logging.getLogger('krotov').info(
        "row split %d: the %s sweep timed out (%s); redoing it, and going on, with one workgroup per objective",
        engine.row_split, what, exc)
    engine.set_row_split(1)


def _attempt(sweep):
    """``(result, None)`` of a sweep that got through, ``(None, error)`` of one that timed out or cannot be resident."""
    try:
        return sweep(), None
    except KrotovHipError as exc:
        if exc.code not in (KH_ERR_TIMEOUT, KH_ERR_UNSUPPORTED):
            raise
        return None, exc


class UpdateLadder:
    """The retry policy of one engine's single-launch update sweep, and all it remembers from sweep to sweep."""

    def __init__(self, engine):
        self.engine = engine
        self.single_launch = True  # until the single-launch update sweep has failed for good
        self.strikes = 0  # sweeps in a row that ended with one launch per interval
        self.grid = None  # workgroups of the sweep after a retry that got through (None: the engine's choice)
        self.in_a_row = 0  # sweeps in a row on that reduced grid
        self.last_good = None  # the reduced grid that got through the last time the full one timed out

    def run(self, sweep, per_interval):
        """``(opt, psi_T, g_a)`` of ``sweep()`` -- the single-launch update sweep, launched AND checked --, redone on
        smaller grids as far as it takes, or of ``per_interval()``, the form that cannot time out."""
        if not self.single_launch:
            return per_interval()
        eng = self.engine
        grid = self.grid
        if grid is not None and self.in_a_row >= _FULL_GRID_PROBE_EVERY:
            # a co-tenant may have gone away: one sweep on the full grid again (at worst one more timeout)
            eng.set_update_workgroups(0)
            grid, self.in_a_row = None, 0
        rung = 0
        while True:
            out, failure = _attempt(sweep)
            if failure is None:
                break
            if failure.code == KH_ERR_TIMEOUT and getattr(eng, 'row_split', 1) > 1:
                leave_row_split(eng, 'update', failure)  # (no rung: those follow if it times out again)
                continue
            # every rung costs a timed-out sweep (KH_TIMEOUT_MS, 1 s by default): two of them at most -- half the
            # workgroups (what gets through next to a stream holding half of the device), then an eighth -- before the
            # form that cannot time out
            rung += 1
            grid = self._smaller_grid(grid, rung) if rung <= 2 else None
            if grid is None:
                return self._give_up(failure, per_interval)
            logging.getLogger('krotov').warning(
                "single-launch update sweep failed (%s); repeating it on %d workgroups", failure, grid)
        self.strikes = 0
        if grid is not None:
            # a reduced grid got through: it is KEPT (trying the full one first would cost a timed-out sweep per iteration
            # for as long as the co-tenant stays); the full grid gets its chance again after _FULL_GRID_PROBE_EVERY sweeps
            # in a row on the reduced one
            self.in_a_row += 1
            self.last_good = grid
        else:
            self.in_a_row = 0
        self.grid = grid
        return out

    def _smaller_grid(self, grid, rung):
        """The grid the engine grants on rung 1 or 2 below ``grid`` (None: its own), or None if there is no smaller one."""
        eng = self.engine
        try:
            full = eng.set_update_workgroups(0)
            if grid is None and self.last_good is not None and self.last_good < full:
                nxt = self.last_good  # (what got through the last time this happened)
            else:
                nxt = (grid if grid is not None else full) // (2 if rung == 1 else 4)
            return eng.set_update_workgroups(nxt) if nxt >= 1 else None
        except KrotovHipError as refusal:
            if refusal.code != KH_ERR_UNSUPPORTED:
                raise
            return None

    def _give_up(self, failure, per_interval):
        """``failure``: the last error of the sweep itself.  One launch per interval, this time or from here on."""
        # back to the engine's own grid, in the engine AND in what this object remembers of it
        self.engine.set_update_workgroups(0)
        self.grid, self.in_a_row, self.last_good = None, 0, None
        self.strikes += 1
        # a co-tenant may go away, but not after three sweeps in a row
        if failure.code == KH_ERR_UNSUPPORTED or self.strikes >= 3:
            self.single_launch = False
        logging.getLogger('krotov').warning(
            "single-launch update sweep failed (%s); repeating it with one launch per interval%s", failure,
            "" if self.single_launch else " (and staying with that form)")
        return per_interval()
