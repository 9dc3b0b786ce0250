"""ctypes mirror of `include/brax_amd_mlp_group.h`: the group forms of the
learner MLP entry points, a table of named signatures as `abi.ARGS` is for
`include/brax_amd.h` (`tests/test_mlp_group.py` checks it against the header).
"""
import ctypes as C

from brax_amd import abi

MLP_MAX_GROUP = 8  # BX_MLP_MAX_GROUP


class BxMlpMember(C.Structure):
  """One member of a group: a whole bx_mlp_forward / bx_mlp_backward problem.
  A None `dy` keeps the member out of the backward launches."""
  _fields_ = [('net', C.POINTER(abi.BxMlp)), ('rows', C.c_int64), ('x', C.c_void_p),
              ('x_stride', C.c_int64), ('y', C.c_void_p), ('saved', C.c_void_p),
              ('dy', C.c_void_p), ('dx', C.c_void_p), ('grads', C.POINTER(abi.BxMlpGrads)),
              ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64)]


_members = ('members', C.POINTER(BxMlpMember))
ARGS = {
    'bx_mlp_group_sizes': (('member_bytes', C.POINTER(C.c_int32)),),
    'bx_mlp_group_forward': (_members, ('n_members', C.c_int32), ('stream', C.c_void_p)),
    'bx_mlp_group_backward': (_members, ('n_members', C.c_int32), ('query', C.c_int32),
                              ('stream', C.c_void_p)),
}
SIGNATURES = {name: ([t for _, t in args], C.c_int) for name, args in ARGS.items()}
