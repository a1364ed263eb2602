"""Latency of a stream feed: the 3x500 unidirectional LSTM CTC network (F 494, C 29) fed chunks of Tc in
{10, 50} frames on S in {1, 16} concurrent streams.  Per shape:
  host_ms     the host clock around Engine.stream_feed (features in host memory to logits in host memory; the call ends in a
              read-back and a synchronise), profiler off: median / min / max over --steps feeds after --warmup
  device_ms   HIP events on the handle's stream around the feed's phases (nasr_set_profiling: pack, input GEMMs, recurrence,
              projection; the launches' gaps inside a phase included, the H2D copy of the chunk and the D2H copy of the logits
              not), profiler off, in further feeds of the same child: median of the sum, and the phases' medians
  kernel_ms   per kernel family, the kernels' own durations per feed from a second child under `rocprofv3 --kernel-trace
              --stats` (the handle's set-up kernels included; tracing lengthens short kernels, so their sum can exceed
              device_ms: it is there to show where a feed's time goes, not how long it is)
  rt_factor   host_ms (and device_ms) over the audio the chunk covers (Tc frames of 10 ms): below 1 the stream keeps up
and, for orientation only, `forward` of the same frames as one batch (B = S, T = Tc, zero initial state) on the per-step
kernels (set_recurrence_mode(0)) on the same box: what the state hand-over adds to a forward pass of that shape.
   python tools/streambench.py [--steps 100 --warmup 10] [--out profiles/stream_bench.json]
With --from-audio every shape also carries "from_audio" (DESIGN.md §16): the same session shape fed SAMPLES
(Engine.stream_feed_audio; 16 kHz, 26 cepstra, numcontext 9, norm_min_frames 50; Tc * 160 samples per slot and feed, which
emit Tc rows each once the first 50 frames are in), measured in the same child as stream_feed of as many rows: host_ms as
above, the front end's device-timed copies and kernels (nasr_featurize_times) and the forward pass's phases.
With --lookahead R (repeatable) the tool measures look-ahead sessions instead: the 3x500 BIDIRECTIONAL concat
network (F 494, C 29), S in {1, 16}, Tc in {10, 50}, every feed Tc new rows per slot behind R held ones, so that each feed
runs a window of Tc + R rows and emits Tc.  Per shape: host_ms and device_ms of Engine.stream_feed_lookahead as above (one
child, no profiler child), and `forward` of Tc + R frames as one batch on the per-step kernels in the same process: a feed
recomputes its R look-ahead rows, so that forward pass is what it is expected to cost.
   python tools/streambench.py --lookahead 20 --lookahead 50 [--out profiles/stream_lookahead_bench.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

F, H, L, C = 494, 500, 3, 29
SHAPES = [(1, 10), (1, 50), (16, 10), (16, 50)]
FRAME_MS = 10.0          # winstep of the front end


def worker(a):
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.networks.hipnetwork import _glorot_init
    S, Tc = (int(x) for x in a.worker.split('x'))
    e = Engine(F, H, L, False, 'none', C)
    e.set_params(_glorot_init(e.tensors(), 1))
    mode = e.recurrence_mode
    rs = np.random.RandomState(7)
    chunks = [rs.randn(S, Tc, F).astype(np.float32) for _ in range(4)]
    n = [Tc] * S
    ms = {'stream_feed': [], 'forward_per_step': []}
    e.stream_open(S)
    for i in range(a.warmup + a.steps):
        x = chunks[i % 4]
        t0 = time.perf_counter()
        out = e.stream_feed(x, n)
        if i >= a.warmup:
            ms['stream_feed'].append((time.perf_counter() - t0) * 1e3)
    assert np.isfinite(out).all() and e.stream_frames().tolist() == [(a.warmup + a.steps) * Tc] * S
    dev = []
    if not a.profiled:
        e.set_profiling(True)
        for i in range(a.steps):
            e.stream_feed(chunks[i % 4], n)
            pt = e.phase_times()
            dev.append([pt['pack_ms'], pt['xproj_ms'], pt['rec_fwd_ms'], pt['proj_ctc_ms']])
        e.set_profiling(False)
    e.stream_close()
    audio = None
    if a.from_audio and not a.profiled:
        audio = from_audio(a, e, S, Tc)
    if not a.profiled:      # (kept out of the profiled child: its kernel statistics are the feeds' alone)
        e.set_recurrence_mode(False)
        for i in range(a.warmup + a.steps):
            x = chunks[i % 4]
            t0 = time.perf_counter()
            e.forward(x, n)
            if i >= a.warmup:
                ms['forward_per_step'].append((time.perf_counter() - t0) * 1e3)
    res = {'S': S, 'Tc': Tc, 'feeds': a.warmup + a.steps, 'recurrence_mode_of_the_handle': mode,
           'host_ms': {k: {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
                       for k, v in ms.items() if v}}
    if audio:
        res['from_audio'] = audio
    if dev:
        dev = np.asarray(dev)
        res['device_ms_per_feed'] = round(float(np.median(dev.sum(1))), 4)
        res['device_ms_by_phase'] = dict(zip(('pack', 'input_gemms', 'recurrence', 'projection'),
                                             (round(float(x), 4) for x in np.median(dev, 0))))
    print('STREAMBENCH ' + json.dumps(res), flush=True)
    e.close()


def worker_lookahead(a):
    """one look-ahead shape SxTcxR in steady state: every feed a window of Tc + R rows"""
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.networks.hipnetwork import _glorot_init
    S, Tc, R = (int(x) for x in a.worker.split('x'))
    e = Engine(F, H, L, True, 'concat', C)
    e.set_params(_glorot_init(e.tensors(), 1))
    mode = e.recurrence_mode
    rs = np.random.RandomState(7)
    chunks = [rs.randn(S, Tc, F).astype(np.float32) for _ in range(4)]
    n = [Tc] * S
    e.stream_open_lookahead(S, R)
    fill = rs.randn(S, R, F).astype(np.float32)
    assert e.stream_feed_lookahead(fill, [R] * S)[1].tolist() == [0] * S          # R rows held: from here on a feed emits Tc
    host, dev = [], []
    for i in range(a.warmup + 2 * a.steps):
        if i == a.warmup + a.steps:
            e.set_profiling(True)
        t0 = time.perf_counter()
        out, rows = e.stream_feed_lookahead(chunks[i % 4], n)
        dt = (time.perf_counter() - t0) * 1e3
        assert rows.tolist() == n
        if a.warmup <= i < a.warmup + a.steps:
            host.append(dt)
        elif i >= a.warmup + a.steps:
            pt = e.phase_times()
            dev.append([pt['pack_ms'], pt['xproj_ms'], pt['rec_fwd_ms'], pt['proj_ctc_ms']])
    e.set_profiling(False)
    assert np.isfinite(out).all() and e.stream_frames().tolist() == [(a.warmup + 2 * a.steps) * Tc] * S
    e.stream_close()
    e.set_recurrence_mode(False)
    win = [rs.randn(S, Tc + R, F).astype(np.float32) for _ in range(4)]
    fwd = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        e.forward(win[i % 4], [Tc + R] * S)
        if i >= a.warmup:
            fwd.append((time.perf_counter() - t0) * 1e3)
    dev = np.asarray(dev)

    def stat(v):
        return {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    res = {'S': S, 'Tc': Tc, 'R': R, 'window_rows': Tc + R, 'feeds': a.warmup + 2 * a.steps, 'recurrence_mode_of_the_handle': mode,
           'host_ms': {'stream_feed_lookahead': stat(host), 'forward_per_step_of_the_window': stat(fwd)},
           'device_ms_per_feed': round(float(np.median(dev.sum(1))), 4),
           'device_ms_by_phase': dict(zip(('pack', 'input_gemms', 'recurrence', 'projection'),
                                          (round(float(x), 4) for x in np.median(dev, 0)))),
           'audio_ms_per_chunk': Tc * FRAME_MS, 'latency_ms_of_the_rule': (Tc + R) * FRAME_MS}
    res['rt_factor_host'] = round(res['host_ms']['stream_feed_lookahead']['median'] / (Tc * FRAME_MS), 4)
    res['feed_over_forward_host'] = round(res['host_ms']['stream_feed_lookahead']['median'] / res['host_ms']['forward_per_step_of_the_window']['median'], 3)
    print('STREAMBENCH ' + json.dumps(res), flush=True)
    e.close()


def from_audio(a, e, S, Tc):
    """the session fed samples: host clock, then with the profiler on the front end's and the forward pass's device time"""
    from neuralasr_amd.features import Featurizer
    sr, numcep, nc, M = 16000, 26, 9, 50
    fz = Featurizer(sr, numcep, nc, normalization='causal', norm_min_frames=M)
    assert fz.width == F
    step = fz.frame_params()[1]
    rs = np.random.RandomState(8)
    feeds = a.warmup + 2 * a.steps
    audio = (0.1 * rs.randn(S, fz.frame_params()[0] + (M + nc) * step + feeds * Tc * step)).astype(np.float32)
    e.stream_open(S)
    e.stream_attach_audio(fz)
    pos = fz.frame_params()[0] + (M + nc - 1) * step          # the first M + nc frames: from here on Tc * step samples emit Tc rows
    e.stream_feed_audio([audio[b, :pos] for b in range(S)])
    host, front, dev = [], [], []
    for i in range(feeds):
        if i == a.warmup + a.steps:
            e.set_profiling(True)
        chunk = [audio[b, pos:pos + Tc * step] for b in range(S)]
        pos += Tc * step
        t0 = time.perf_counter()
        out, rows = e.stream_feed_audio(chunk)
        dt = (time.perf_counter() - t0) * 1e3
        assert rows.tolist() == [Tc] * S and np.isfinite(out).all()
        if a.warmup <= i < a.warmup + a.steps:
            host.append(dt)
        elif i >= a.warmup + a.steps:
            pt = e.phase_times()
            t = fz.times()
            front.append([t[0], t[1]])
            dev.append(pt['pack_ms'] + pt['xproj_ms'] + pt['rec_fwd_ms'] + pt['proj_ctc_ms'])
    e.set_profiling(False)
    e.stream_close()
    fz.close()
    front = np.median(np.asarray(front), 0)
    return {'samples_per_slot_and_feed': Tc * step, 'norm_min_frames': M,
            'host_ms': {'median': round(float(np.median(host)), 3), 'min': round(min(host), 3), 'max': round(max(host), 3)},
            'front_end_copies_ms': round(float(front[0]), 4), 'front_end_kernels_ms': round(float(front[1]), 4),
            'forward_device_ms': round(float(np.median(dev)), 4)}


def kernel_ns(d):
    """(total device ns of all kernels, {kernel family: ns}) of a profiled child"""
    total, fam = 0, {}
    for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                ns = int(row['TotalDurationNs'])
                total += ns
                name = row['Name'].split('(')[0].split('<')[0].split('::')[-1].split(' ')[-1]
                fam[name] = fam.get(name, 0) + ns
    return total, fam


def child(shape, a, profiled, d=None):
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', 'x'.join(str(x) for x in shape), '--steps', str(a.steps),
           '--warmup', str(a.warmup)]
    if a.from_audio and not profiled:
        cmd.append('--from-audio')
    if profiled:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--'] + cmd + ['--profiled']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    line = [l for l in r.stdout.splitlines() if l.startswith('STREAMBENCH ')]
    if r.returncode != 0 or not line:
        raise SystemExit('the %s child failed (%d):\n%s\n%s' % ('x'.join(str(x) for x in shape), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(line[0][len('STREAMBENCH '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_bench.json'))
    ap.add_argument('--from-audio', action='store_true', help='also feed the session samples (stream_feed_audio)')
    ap.add_argument('--worker', help='(internal) SxTc: the measured process of one shape')
    ap.add_argument('--profiled', action='store_true', help='(internal) the child runs under the profiler')
    ap.add_argument('--lookahead', type=int, action='append', metavar='R',
                    help='measure look-ahead sessions of the bidirectional 3x500 network with R look-ahead frames (repeatable)')
    a = ap.parse_args()
    if a.worker:
        return worker_lookahead(a) if a.worker.count('x') == 2 else worker(a)
    if a.lookahead:
        doc = {'tool': 'tools/streambench.py --lookahead', 'network': 'bilstm 3x500 concat, F %d, C %d' % (F, C),
               'method': 'host clock and HIP events (nasr_set_profiling) in one child per shape; every feed runs a window of Tc + R rows',
               'shapes': []}
        for S, Tc in SHAPES:
            for R in a.lookahead:
                res = child((S, Tc, R), a, False)
                doc['shapes'].append(res)
                print(json.dumps(res), flush=True)
        out = a.out if a.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'stream_lookahead_bench.json')
        with open(out, 'w') as fh:
            json.dump(doc, fh, indent=1)
            fh.write('\n')
        return
    doc = {'tool': 'tools/streambench.py', 'network': 'lstm_ctc_net 3x500 uni, F %d, C %d' % (F, C),
           'method': 'host clock and HIP events in one child per shape; kernel durations from a second child under rocprofv3 --kernel-trace --stats',
           'shapes': []}
    for shape in SHAPES:
        res = child(shape, a, False)
        with tempfile.TemporaryDirectory() as d:
            prof = child(shape, a, True, d)
            total, fam = kernel_ns(d)
        feeds = prof['feeds']
        audio_ms = shape[1] * FRAME_MS
        res['kernel_ms_per_feed_profiled'] = round(total / feeds / 1e6, 3)
        res['kernel_ms_by_kernel_profiled'] = {k: round(v / feeds / 1e6, 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])[:8]}
        res['audio_ms_per_chunk'] = audio_ms
        res['rt_factor_host'] = round(res['host_ms']['stream_feed']['median'] / audio_ms, 4)
        res['rt_factor_device'] = round(res['device_ms_per_feed'] / audio_ms, 4)
        if 'from_audio' in res:
            res['from_audio']['feed_audio_over_feed_host'] = round(res['from_audio']['host_ms']['median'] / res['host_ms']['stream_feed']['median'], 3)
        res['feed_over_forward_host'] = round(res['host_ms']['stream_feed']['median'] / res['host_ms']['forward_per_step']['median'], 3)
        doc['shapes'].append(res)
        print(json.dumps(res), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
