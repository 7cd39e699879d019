"""The burst timing tap's definition against planted truth, on the CPU: the float64 model (tests/toa_model.py) over the oracle's own
decimated stream of synthetic bursts whose positions and carrier offsets are known.  No GPU and nothing of the library but the
template: what is proved here is that the definition measures what it says, the GPU tests prove that the kernel computes it."""
import numpy as np
import pytest

import toa_model as tm
from dumpvdl2_amd import synth, vdl2hip
from oracle import pyoracle

OS = 10
FREQ = 136975000


@pytest.fixture(scope="module")
def run():
    """seed 7, oversample 10, one channel, noise-free, through the oracle's channel filter -> per burst the model's position, the
    planted one, the model's carrier offset and the planted one"""
    cfg = synth.SynthConfig(centerfreq=FREQ, freqs=(FREQ,), oversample=OS, duration_s=9.0, seed=7, noise_sigma=0.0)
    iq, bursts = synth.synthesize(cfg, dtype=np.int16)
    o = pyoracle.Oracle(FREQ, [FREQ], oversample=OS)
    n_dec = iq.size // 2 // OS
    tr = o.trace(0, n_dec)
    o.process(iq.tobytes())
    y = tr[:, 0].astype(np.float64) + 1j * tr[:, 1].astype(np.float64)
    ppm = {f["sync_sample"]: f["ppm_error"] for f in o.frames()}
    o.close()
    s32 = vdl2hip.toa_template()
    sps = synth.SPS * OS
    rows = []
    for b in bursts:
        planted = (b.start_sample + (4 + 5) * sps) / OS                      # modulate(): a span of 4 symbols, 5 ramp-up symbols, then symbol 0
        t0 = int(round(planted)) + 2                                          # an anchor as a decoder's clock would give it: within a sample or two
        # the slope the decoder used for this burst (demod.c:185 backwards), and the slope the burst really has
        near = [v for k, v in ppm.items() if abs(k - (planted + 150)) < 40]
        assert near, f"the oracle decoded nothing of the burst at {planted}"
        row = dict(planted=planted, cfo_planted=b.cfo_hz)
        for name, dphi in (("decoder", np.float32(near[0] * 1e-6 * FREQ * 2.0 * np.pi / 10500.0)), ("true", np.float32(b.cfo_hz * 2.0 * np.pi / 10500.0))):
            W = 8
            yw = tm.window(lambda first, count: y[first:first + count], t0, W)
            m = tm.correlate(s32, yw, dphi, W)
            d = tm.derive(m["P"].astype(np.float32), W, t0, dphi, 1.0, 1.0, 0.0)
            kp = d["kp"]
            resid = float(np.angle(m["cb"][kp] * np.conj(m["ca"][kp]))) / tm.HALF
            row[name] = dict(pos=d["peak_sample"] + float(d["toa_frac"]), flags=d["flags"], slope_hz=float(dphi) / 10.0 * 105000.0 / (2.0 * np.pi),
                             cfo=(float(dphi) / 10.0 + resid) * 105000.0 / (2.0 * np.pi))
        rows.append(row)
    return rows


def stats(rows, name):
    off = np.array([r[name]["pos"] - r["planted"] for r in rows])
    return off, f"{off.size} bursts, {name} slope: mean offset {off.mean():.4f} samples, spread {off.max() - off.min():.4f}, std {off.std():.4f}, min {off.min():.4f} max {off.max():.4f}"


def test_position_spread(run):
    """The spread (max - min over the bursts) of model position - planted position is at most 0.05 sample: three times the 0.0152 the
    definition's author measured on this run, because the set of bursts changes if the synthesiser ever does.  That figure is the
    estimator's own: it is reproduced with the slope each burst really has.
    Measured here, 28 bursts: mean offset 2.3012 samples (the channel filter's delay at oversample 10 - the figure vdl2hip.h quotes),
    spread 0.0143, standard deviation 0.0040.
    With the slope the decoder used instead - up to 24 Hz off on this run - the mean is 2.3033, the spread 0.2807 and the standard
    deviation 0.0836: the unique word's waveform is not symmetric, so a slope that is off by 1 Hz moves the peak by -0.0057 sample
    (the fit over these bursts).  That is printed, and quoted in vdl2hip.h, not asserted: it is the decoder's error, not the tap's."""
    off, line = stats(run, "true")
    print(line)
    off_d, line = stats(run, "decoder")
    print(line)
    err = np.array([r["decoder"]["slope_hz"] - r["cfo_planted"] for r in run])
    print(f"decoder's slope error: largest {np.abs(err).max():.1f} Hz; position against it: {np.polyfit(err, off_d, 1)[0]:+.4f} sample per Hz")
    assert off.size >= 10 and all(r["true"]["flags"] == 0 and r["decoder"]["flags"] == 0 for r in run)
    assert off.max() - off.min() <= 0.05


def test_carrier_offset(run):
    """|cfo_hz - planted| stays under 40 Hz on this run, with the slope the decoder used (up to 24 Hz off).  Measured here with the
    model, 28 bursts: largest error 12.95 Hz, mean -2.98 Hz, standard deviation 6.82 Hz - the half-sum phase difference takes back
    about half of the decoder's error; what is left is the data-like structure of the two halves.  The cap is three times the largest,
    for the same reason as the position's."""
    err = np.array([r["decoder"]["cfo"] - r["cfo_planted"] for r in run])
    print(f"{err.size} bursts: cfo error mean {err.mean():+.2f} Hz, std {err.std():.2f}, largest {np.abs(err).max():.2f}")
    assert err.size >= 10
    assert np.abs(err).max() <= 40.0
