"""The parameter set shared by test_adamw_host.py and test_gpu_adamw.py: the smallest shapes at which
each path of the AdamW kernels can go wrong.

Conv weights (K, C, R, S), stride, what they exercise:
  (40, 3, 3, 3)   C not a multiple of 4 (scalar staging), C padded to 8, partial 32-row tile
  (32, 32, 3, 3)  exact 32x32 tile
  (3, 32, 1, 1)   K padded to 8, odd K in the pair writes of wt
  (72, 68, 1, 1)  crosses the 64x64 tile on both axes
  (16, 8, 7, 7)   49 taps (16x8 tile)
  (24, 16, 3, 3)  stride 2: the parity-class dgrad layout
  (8, 8, 9, 9)    81 taps: registered but not fusable (plain block + refresh())
Plain tensors: (32,), (1,), (2049,) (crosses a 2048-element block, tail not a multiple of 4), and (37,)
whose gradient is a view 4 bytes into its storage (the misaligned path).
"""
import ctypes

CONVS = [((40, 3, 3, 3), (1, 1), (1, 1)), ((32, 32, 3, 3), (1, 1), (1, 1)), ((3, 32, 1, 1), (1, 1), (0, 0)),
         ((72, 68, 1, 1), (1, 1), (0, 0)), ((16, 8, 7, 7), (1, 1), (3, 3)), ((24, 16, 3, 3), (2, 2), (1, 1)),
         ((8, 8, 9, 9), (1, 1), (4, 4))]
PLAIN = [(32,), (1,), (2049,), (37,)]
MISALIGNED = len(CONVS) + 3  # index of the (37,) tensor in CONVS + PLAIN
NO_GRAD_AT_STEP2 = len(CONVS) + 0  # the parameter left without a grad at step 2 (its step number diverges)
STEPS = 12


def ceil8(n):
    return (n + 7) // 8 * 8


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class SgdParam(ctypes.Structure):  # mx_sgd_param
    _fields_ = [("p", ctypes.c_void_p), ("buf", ctypes.c_void_p), ("n", ctypes.c_int64), ("first", ctypes.c_int32),
                ("pack", ctypes.c_int32)]


class AdamwParam(ctypes.Structure):  # mx_adamw_param
    _fields_ = [("p", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("pack", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def gradient(torch, shape, step, index):
    """The gradient of tensor `index` at `step` (CPU f32): randn * 10**e with e drawn from -6..0 per
    element, about 10 % of the elements exactly 0 -- v near 0 and the eps branch, inside the normal
    f32 range."""
    g = torch.Generator().manual_seed(1000 * step + index)
    x = torch.randn(shape, generator=g)
    e = torch.randint(-6, 1, shape, generator=g).float()
    x = x * torch.pow(torch.tensor(10.0), e)
    x[torch.rand(shape, generator=g) < 0.1] = 0.0
    return x


def initial(torch, shape, index):
    g = torch.Generator().manual_seed(77 + index)
    return torch.randn(shape, generator=g) * 0.1
