"""``run_until_finished`` -- replay a captured step until every system of the batch has reached its end time.

Under an adaptive dt every system keeps its own clock on the device and reaches a given time after its own number of steps.
With ``StepDraw.set_end_time`` a system that has reached its end rests -- its rows carry ``skip``, nothing of it moves -- so
the replays that the slowest system still needs leave the others where they stopped, and the host only has to learn WHEN all
are done.  That takes one small copy per chunk of replays, not one read of B clocks per step::

    draw.set_end_time(t_end)                 # before the capture
    ledger.set_time_rule(period_ps * to_time_units)
    with torch.cuda.graph(graph):
        draw.fill(); integrator.step_one(); ...; ledger.record(); thermostat.step_async()
    replays = run_until_finished(graph.replay, draw)
    draw.state()["elapsed"]                  # every clock is >= t_end; draw.state()["draws"]: the steps each system took
"""
from __future__ import annotations


def run_until_finished(replay, draw, check_every: int = 256, max_replays=None) -> int:
    """Calls ``replay()`` in chunks of ``check_every`` and asks ``draw`` (a ``StepDraw`` with end times) once per chunk, behind
    one synchronisation, how many systems are at rest; returns the number of replays made once all are, or at ``max_replays``
    (None: no limit).  The return is therefore the first chunk end at or past the last system's finish (a system is counted
    from the replay AFTER the one that carried its clock past the end: that is the ``fill()`` which puts it to rest).
    Replays past a system's finish do not change it.  A system without an end time never finishes: give ``max_replays``."""
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError("run_until_finished: check_every is at least 1")
    if max_replays is not None and int(max_replays) < 0:
        raise ValueError("run_until_finished: max_replays is None or not negative")
    done = 0
    while draw.n_finished() < draw.n_systems:
        chunk = check_every if max_replays is None else min(check_every, int(max_replays) - done)
        if chunk <= 0:
            break
        for _ in range(chunk):
            replay()
        done += chunk
    return done
