"""Scripted loss sequences for the update tests: tests/test_update_reference_cpu.py proves them on the float64 reference and on torch's
schedulers, tests/test_gpu_update_kernel.py injects the same scripts into the engine's update kernel."""
import numpy as np

# cosine restarts with T_0 = 200, T_mult = 2: cycles start at 200, 600, 1400, 3000, 6200, ... -- both sides of 200, 600 and 3000, a loss
# far below T_0 and one eight cycles up; T_mult = 1: both sides of 200, 400 and 1000
COSINE_T2 = [0.37, 150.0, 199.5, 250.0, 599.0, 601.0, 1000.0, 2999.0, 3001.0, 1e5, 12.5, 1399.0, 1401.0, 6199.0, 6201.0, 3.0, 199.0, 201.0,
             450.0, 75.0, 0.01, 5000.0, 100.0, 2500.0, 320.0, 1.5, 880.0, 40.0, 199.9, 200.5, 64.0, 1e4, 7.0, 598.0, 2.0, 1.0, 0.5, 0.25,
             0.125, 0.0625]
COSINE_T1 = [0.37, 150.0, 199.5, 200.5, 250.0, 399.0, 401.0, 999.0, 1001.0, 1e5 + 3.0, 12.5, 599.0, 601.0, 3.0, 199.0, 201.0, 450.0, 75.0,
             0.01, 5000.5, 100.0, 2500.25, 320.0, 1.5, 880.0, 40.0, 799.5, 800.5, 64.0, 10001.0, 7.0, 598.0, 2.0, 1.0, 0.5, 0.25, 0.125,
             0.0625, 1234.0, 4321.0]
# plateau, patience 3, factor 0.5, min_lr 2e-4, relative threshold 1e-4, lr0 = 1e-3:
#   1.0 best; 0.99989 improves (just inside 1 - 1e-4); 0.99980 does NOT (0.99989 (1 - 1e-4) = 0.999790011: just outside) -> bad 1;
#   three more bad -> bad 4 > 3: 5e-4; 0.5 improves; four bad: 2.5e-4; four bad: max(1.25e-4, 2e-4) = 2e-4 (the clamp);
#   four bad: new lr = lr, no change, num_bad back to 0; 0.4 improves; four bad again: still 2e-4
PLATEAU = ([1.0, 0.99989, 0.99980, 1.2, 1.1, 0.9999] + [0.5] + [0.6, 0.7, 0.55, 0.50001] + [0.8, 0.9, 0.49996, 0.51] +
           [0.52, 0.53, 0.54, 0.55] + [0.4] + [0.41, 0.42, 0.43, 0.44] + [0.45, 0.39998, 0.46, 0.47] + [0.3, 0.31, 0.32, 0.33, 0.34, 0.35, 0.36] + [0.2, 0.21, 0.22, 0.23, 0.24])
PLATEAU_KW = dict(patience=3, factor=0.5, min_lr=2e-4, threshold=1e-4)


def f32(x):
    return float(np.float32(x))
