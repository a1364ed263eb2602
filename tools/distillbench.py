"""What distillation costs per step: the 3x500 bidirectional concat student (F 494, C 29) trained in
windows of (C, R) = (50, 20) and a whole-utterance 3x500 teacher at B 16, T 500, every utterance full length, both on one
stream as HipNetwork runs them, timed in ONE process in configurations that take turns:
  student_alone        the student's step with distillation off (compute_grads + apply_adam)
  student_distilled    what a distilled training step enqueues: the teacher's forward pass, nasr_take_teacher_logits, the
                       student's step with the term
  term_only            the student's step with the term on teacher logits taken once: the term's kernels alone
  teacher_forward      the teacher's forward pass alone
A turn times --steps steps with the host clock between two synchronisations (the batches stay resident: uploads are not
part of it).  --rounds turns per configuration, interleaved, so that clock and thermal drift hit all alike; reported: the
median over the turns of the per-step time, its min and max, and the difference to student_alone's median.
   python tools/distillbench.py [--rounds 5 --steps 10 --warmup 3] [--out profiles/distill_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

F, H, L, C = 494, 500, 3, 29
CHUNK = (50, 20)
WEIGHT, TAU = 0.5, 2.0
CONFIGS = ['student_alone', 'student_distilled', 'term_only', 'teacher_forward']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.networks.hipnetwork import _glorot_init
    from oracle import nasr_oracle as O
    spec = O.ModelSpec(F, H, L, True, 'concat', C)
    feats, seq_len, labels, label_len = O.synth_batch(spec, a.batch, a.frames, seed=3, var_len=False, Lmin=20, Lmax=60)
    feats = feats.astype(np.float32)
    stream = torch.cuda.Stream(device=0)
    student = Engine(F, H, L, True, 'concat', C, learning_rate=1e-4, stream=stream.cuda_stream)
    teacher = Engine(F, H, L, True, 'concat', C, learning_rate=1e-4, stream=stream.cuda_stream)
    student.set_params(_glorot_init(student.tensors(), 1))
    teacher.set_params(_glorot_init(teacher.tensors(), 2))
    student.set_chunking(*CHUNK)
    student.upload_batch(feats, seq_len, labels, label_len)
    teacher.upload_batch(feats, seq_len, None, None)
    B, T = a.batch, a.frames
    ms = {name: [] for name in CONFIGS}
    parts = {}

    def student_step():
        student.compute_grads()
        student.apply_adam(1.0)

    def turn(name, steps, record):
        student.set_distill(0.0 if name in ('student_alone', 'teacher_forward') else WEIGHT, TAU)
        if name == 'term_only':
            teacher.forward_resident(B, T, fetch=False)
            student.take_teacher_logits(teacher)
        student.synchronize()
        teacher.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if name in ('student_distilled', 'teacher_forward'):
                teacher.forward_resident(B, T, fetch=False)
            if name == 'student_distilled':
                student.take_teacher_logits(teacher)
            if name != 'teacher_forward':
                student_step()
        student.synchronize()
        teacher.synchronize()
        per = (time.perf_counter() - t0) * 1e3 / steps
        if record:
            ms[name].append(per)
            if name != 'teacher_forward':
                parts[name] = [float(x) for x in (student.get_loss(),) + student.distill_loss()]

    for name in CONFIGS:
        turn(name, a.warmup, False)
    for _ in range(a.rounds):
        for name in CONFIGS:
            turn(name, a.steps, True)
    kinds = {'student': student.recurrence_mode, 'teacher': teacher.recurrence_mode}
    student.close()
    teacher.close()
    base = float(np.median(ms['student_alone']))
    res = {'network': '3x500 bidirectional concat, F %d, C %d; student in windows of (C, R) = %s, teacher whole-utterance' % (F, C, CHUNK),
           'B': B, 'T': T, 'weight': WEIGHT, 'temperature': TAU, 'recurrence_kinds': kinds, 'rounds': a.rounds,
           'steps_per_turn': a.steps, 'configs': {}}
    for name in CONFIGS:
        v = ms[name]
        res['configs'][name] = {'step_ms': {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)},
                                'minus_student_alone_ms': round(float(np.median(v)) - base, 3)}
        if name in parts:
            res['configs'][name]['last_loss_ctc_kd'] = parts[name]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
