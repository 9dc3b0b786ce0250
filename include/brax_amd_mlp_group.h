/*
 * brax_amd — the learners' MLPs in groups: several networks in ONE forward
 * launch and at most TWO backward launches (brax_amd.h: bx_mlp_forward /
 * bx_mlp_backward take exactly one).
 *
 * The declarations live in a header of their own, on top of brax_amd.h, whose
 * conventions hold here unchanged. (Additive: no ABI bump.)
 */
#ifndef BRAX_AMD_MLP_GROUP_H_
#define BRAX_AMD_MLP_GROUP_H_

#include "brax_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A group is 1 .. BX_MLP_MAX_GROUP members, each a complete problem of its
 * own: its own network (the shapes may differ between members), rows, x and
 * outputs, as bx_mlp_forward and bx_mlp_backward take them for one network.
 * Members may share an x, or weights. The forward launch has one workgroup
 * per (member, 32-row tile); backward launch (i) the same; launch (ii) one per
 * (member, layer, 32 x 64 tile of dW). A tile runs the code of the
 * single-network kernels in their order, so every output of a member is bit
 * for bit what bx_mlp_forward / bx_mlp_backward write for that member alone. */
#define BX_MLP_MAX_GROUP 8
typedef struct bx_mlp_member {
  const bx_mlp* net;
  int64_t rows;
  const float* x;
  int64_t x_stride;
  float* y;     /* forward */
  float* saved; /* forward: written (NULL: not wanted); backward: read */
  const float* dy; /* backward; NULL: the member takes no part in it */
  float* dx;       /* NULL: not wanted */
  const bx_mlp_grads* grads; /* NULL: none */
  void* workspace;           /* the member's own, as bx_mlp_backward's */
  int64_t workspace_bytes;
} bx_mlp_member;

/* sizeof(bx_mlp_member) as the library was compiled */
int bx_mlp_group_sizes(int32_t* member_bytes);

/* bx_mlp_forward for every member in ONE launch; reads net, rows, x,
 * x_stride, y and saved of each. A member with rows = 0 contributes no
 * workgroups. A null `members`, n_members outside 1 .. BX_MLP_MAX_GROUP, any
 * failure of bx_mlp_forward for a member (the message prefixed `member <i>: `),
 * or two members that name the same y or the same non-null saved fail before
 * any device call. */
int bx_mlp_group_forward(const bx_mlp_member* members, int32_t n_members, void* stream);

/* bx_mlp_backward for every member with a non-null dy, in at most TWO
 * launches: (i) for the members that want dx or a hidden layer's gradient,
 * (ii) for those that want a parameter gradient; either is left out when no
 * member needs it. Each member's workspace is its own, of workspace_bytes
 * bytes, 16-byte aligned. With query != 0 the call launches nothing, checks
 * each member's network and rows alone and writes the size each needs to its
 * workspace_bytes: max(16, 4 * rows * H). The failures of
 * bx_mlp_group_forward and of bx_mlp_backward per member (prefixed likewise),
 * and two members that name the same dx, workspace, dw or db entry fail before
 * any device call. */
int bx_mlp_group_backward(bx_mlp_member* members, int32_t n_members, int32_t query, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BRAX_AMD_MLP_GROUP_H_ */
