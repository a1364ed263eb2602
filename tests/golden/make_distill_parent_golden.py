"""Generates tests/golden/distill_parent.json: SHA-256 digests of the last checkpoint that `python -m neuralasr_amd.train`
writes on the toy sample set (tests/golden/sample_set) from a config WITHOUT the distillation keys.
tests/test_gpu_distill.py runs the same loop and compares: a tree with the feature must train, with the feature off, to the
bits of the commit before it.  Run it on an MI355X with that commit built
(`python tests/golden/make_distill_parent_golden.py`); a mismatch is fixed in the code, never by running this again.

Only data is written.  The loop helpers here (loop_config, run_loop) use the package's public calls only and are what the
test imports, so both run the very same loop."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'distill_parent.json')
SAMPLES = os.path.join(HERE, 'sample_set')
NET = 'networks.lstm_ctc_net.SmallLstmCTCNet'       # 1 x 128, unidirectional: a CTC network that may learn and teach


def loop_config(d, epochs=3, start_step=0, model='model', learningrate=None, **extra):
    """toy.config re-rooted at this checkout for a run in directory d: one tower, batches of 4 (two per epoch), a log line
    and a checkpoint every 2 steps; `extra`: more [Parameters] keys"""
    over = {'output': SAMPLES, 'model_dir': os.path.join(str(d), model), 'network': NET, 'num_gpus': 1, 'batch_size': 4,
            'epochs': epochs, 'start_step': start_step}
    if learningrate is not None:
        over['learningrate'] = learningrate
    out = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        key = ln.split('=')[0]
        out.append('%s=%s' % (key, over[key]) if key in over and '=' in ln else ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    path = os.path.join(str(d), '%s.config' % model)
    with open(path, 'w') as f:
        f.write('\n'.join(out) + '\n')
    return path


def run_loop(cfg_path):
    """python -m neuralasr_amd.train <cfg_path>; (the arrays of the last checkpoint, the step it was written at)"""
    from neuralasr_amd import train
    from neuralasr_amd.config import Config
    net = train.main([str(cfg_path)])
    net._settle()
    step = net.global_step
    if getattr(net, '_teacher', None) is not None:
        net._teacher.engine.close()
    net.engine.close()
    with np.load(os.path.join(Config(str(cfg_path), True).model_dir, 'model-%d.npz' % step)) as z:
        return {k: z[k].copy() for k in z.files}, step


def digests(ckpt):
    """SHA-256 of the checkpoint's numeric arrays (floats as float32(x + 0.0) bytes: the sign of an exact zero does not count)"""
    out = {}
    for k in ('params', 'adam_m', 'adam_v'):
        a = np.asarray(ckpt[k]).astype(np.float32) + np.float32(0.0)
        out[k] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out['step'] = int(ckpt['step'])
    return out


def main():
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with tempfile.TemporaryDirectory() as d:
        ckpt, step = run_loop(loop_config(d))
    doc = {'_note': 'SHA-256 of parameters and Adam state after the 6 steps of the plain toy loop (SmallLstmCTCNet, one tower, '
                    'batches of 4, 3 epochs), taken on an MI355X from the commit before distillation was added.  '
                    'tests/golden/make_distill_parent_golden.py',
           'plain': dict(digests(ckpt), global_step=step,
                         params_abs_sum=float(np.abs(np.asarray(ckpt['params'], np.float64)).sum()))}
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(doc['plain']))
    print('wrote', out)


if __name__ == '__main__':
    main()
