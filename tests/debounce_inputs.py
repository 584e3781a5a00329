"""Designed inputs of the debounce tests: burst(8) streams (tests/dense_devices.py: pulses of 20 us, gaps of 20 / 50 us, one
sample per microsecond) with glitches laid where the debounced decode can go wrong.  tests/test_debounce_host.py checks
that the streams are what they say; tests/test_gpu_debounce.py runs them."""
import numpy as np

from tests import dense_devices as dd

GRID = 64                       # samples_per_buffer of the designed streams, and with segment_buffers = 1 a segment of the round form
FULL = (8, 3)                   # minimums at which every glitch below goes, alone
PART = (3, 0)                   # ... at which the pulses of 7 and the dropouts stay


def glitched_burst_runs(nmsg=40, seed=5):
    """(runs with glitches, runs without), equally long: burst(8) messages with pulses of 1, 2 and 7 samples inside bit
    gaps and 30 samples ahead of messages, and dropouts of 1 and 2 samples inside pulses -- never closer than 5 samples
    to a real edge, so at FULL every glitch goes alone and the cleaned stream is the one without.  Behind the messages,
    on the grid of 64 samples the round form's segments start on (no low gap lies whole inside a cut's window there, so
    the cuts stay nominal):
      - a silence with six pulses of 7, each from 3 samples before a multiple of 64: a segment starts inside a deleted
        glitch -- the raw bit in front of it is 1, the cleaned level 0;
      - a level held high with six dropouts of 2, each from 1 sample before a multiple of 64: a segment starts inside
        a deleted gap -- the raw bit in front of it is 0, the cleaned level 1."""
    rng = np.random.default_rng(seed)
    base = dd.burst_runs(8, nmsg, seed=seed)
    runs = [base[0]]
    for i in range(1, len(base)):
        r = base[i]
        if rng.random() < 0.3:
            if i % 2 == 1:                                      # a pulse of 20: a dropout inside
                g = int(rng.integers(1, 3))
                a = int(rng.integers(8, 20 - 8 - g + 1))
            elif r in (20, 50):                                 # a bit gap: a short pulse inside
                g = int(rng.choice([1, 2, 7] if r == 50 else [1, 2]))
                a = int(rng.integers(5, r - 5 - g + 1))
            else:                                               # the pause: a pulse 30 samples ahead of the message
                g = int(rng.choice([1, 2, 7]))
                a = r - 30 - g
            runs += [a, g, r - a - g]
        else:
            runs.append(r)
    assert len(runs) % 2 == 1 and sum(runs) == sum(base)       # the last run is the pause behind the last message: low
    pad = (-sum(runs) - 3) % GRID + GRID
    runs[-1] += pad
    runs += [7, GRID - 7] * 6
    runs[-1] += 13                                              # the high level begins 10 samples behind a multiple
    runs += [GRID - 11] + [2, GRID - 2] * 5 + [2, 30, 202]
    plain = list(base)
    plain[-1] += pad + 6 * GRID + 13
    plain += [GRID - 11 + 5 * GRID + 2 + 30, 202]
    assert sum(runs) == sum(plain)
    return runs, plain
