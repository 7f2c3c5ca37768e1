"""Training nodes, per-row parity: WHAT the host drivers that chain the kernels into autograd nodes compute -- which saved tensor feeds which backward, where a
residual or a direct gradient joins, how the q | k | v slices land in one in_proj, what the CLS row of the last branch layer receives.

  a. the layer node        train_hubert.HubertLayersTrainFn: the no-dropout post-LN body, the pre-LN body (padded, packed), three layers with a frozen layer above a
                           trained one; the pre-LN body with the ViT pair (QuickGELU, no key mask) through the same two body functions
  b. the layer mix         train_hubert.WeightedSumTrainFn, with and without `normalize`
  c. the branch stack      train_branch.BranchStackTrainFn: head dims 64 / 96 / 128, 1 / 2 / 3 layers, post-LN and pre-LN, p = 0 and p = 0.1
  d. the image tower       train_vit.ImageTowerTrainFn on the two tiny towers of tests/vit_train_ref.py

The machinery is that of tests/test_train_mode_parity_gpu.py: fp64 autograd references on the CPU (tests/train_mode_ref.py, tests/train_nodes_ref.py), per row
max|got - ref| / max|ref| for row tensors and the same over the whole tensor for parameter-shaped gradients, bound 4 x MODEL + 1e-3 with MODEL the metric of the
CPU model of a correct implementation (model=True).  `python tools/train_node_bounds.py` prints every value, checks well-posedness and every mutant (a wrong wiring
of the reference must leave the bound); `--emit` prints the MODEL dict below.  Measured on the MI355X: profiles/train_nodes_parity.txt.

Left out of the metrics, and nothing else: the k slice of every q | k | v bias gradient (analytically zero: softmax rows are shift invariant), judged as
tests/test_dropout_gpu.py judges k_b -- norm below 1e-2 of the q slice's; rows >= lens[b], whose gradient must be exactly zero where the node defines it.
Every test asserts how many rows and tensors it judged.  The tool also checks that the zero rule is well-posed: the CPU model's own k slice (it models
delta = dO . O from the stored output, the one source of that slice without dropout) keeps the rule with room for another draw of the rounding noise."""
import dataclasses
import functools

import pytest
import torch

import train_mode_ref as R
import train_nodes_ref as N

BF = torch.bfloat16
F64 = torch.float64

# ---- modelled error of a correct implementation per case and tensor: `python tools/train_node_bounds.py --emit`
MODEL = {
    "node-nodrop-padded/hidden0": 8.01e-03, "node-nodrop-padded/hidden1": 1.75e-02, "node-nodrop-padded/dh_in": 1.13e-02, "node-nodrop-padded/L0.q_w": 5.90e-03,
    "node-nodrop-padded/L0.q_b": 4.49e-03, "node-nodrop-padded/L0.k_w": 6.41e-03, "node-nodrop-padded/L0.v_w": 3.92e-03, "node-nodrop-padded/L0.v_b": 3.07e-03,
    "node-nodrop-padded/L0.o_w": 5.29e-03, "node-nodrop-padded/L0.o_b": 4.71e-03, "node-nodrop-padded/L0.ln1_w": 4.86e-03, "node-nodrop-padded/L0.ln1_b": 3.61e-03,
    "node-nodrop-padded/L0.fc1_w": 5.41e-03, "node-nodrop-padded/L0.fc1_b": 3.41e-03, "node-nodrop-padded/L0.fc2_w": 5.45e-03,
    "node-nodrop-padded/L0.fc2_b": 3.72e-03, "node-nodrop-padded/L0.ln2_w": 5.99e-03, "node-nodrop-padded/L0.ln2_b": 2.57e-03,
    "node-nodrop-padded/L1.q_w": 6.98e-03, "node-nodrop-padded/L1.q_b": 8.87e-03, "node-nodrop-padded/L1.k_w": 6.59e-03, "node-nodrop-padded/L1.v_w": 6.24e-03,
    "node-nodrop-padded/L1.v_b": 5.74e-03, "node-nodrop-padded/L1.o_w": 6.83e-03, "node-nodrop-padded/L1.o_b": 5.38e-03, "node-nodrop-padded/L1.ln1_w": 3.80e-03,
    "node-nodrop-padded/L1.ln1_b": 3.64e-03, "node-nodrop-padded/L1.fc1_w": 4.86e-03, "node-nodrop-padded/L1.fc1_b": 2.54e-03,
    "node-nodrop-padded/L1.fc2_w": 3.30e-03, "node-nodrop-padded/L1.fc2_b": 1.76e-03, "node-nodrop-padded/L1.ln2_w": 3.65e-03,
    "node-nodrop-padded/L1.ln2_b": 0.00e+00,
    "node-nodrop-packed/hidden0": 8.01e-03, "node-nodrop-packed/hidden1": 1.09e-02, "node-nodrop-packed/dh_in": 1.08e-02, "node-nodrop-packed/L0.q_w": 5.58e-03,
    "node-nodrop-packed/L0.q_b": 5.74e-03, "node-nodrop-packed/L0.k_w": 7.35e-03, "node-nodrop-packed/L0.v_w": 5.06e-03, "node-nodrop-packed/L0.v_b": 4.54e-03,
    "node-nodrop-packed/L0.o_w": 4.84e-03, "node-nodrop-packed/L0.o_b": 5.38e-03, "node-nodrop-packed/L0.ln1_w": 4.97e-03, "node-nodrop-packed/L0.ln1_b": 5.56e-03,
    "node-nodrop-packed/L0.fc1_w": 5.25e-03, "node-nodrop-packed/L0.fc1_b": 4.12e-03, "node-nodrop-packed/L0.fc2_w": 3.89e-03,
    "node-nodrop-packed/L0.fc2_b": 2.77e-03, "node-nodrop-packed/L0.ln2_w": 3.61e-03, "node-nodrop-packed/L0.ln2_b": 2.30e-03,
    "node-nodrop-packed/L1.q_w": 8.36e-03, "node-nodrop-packed/L1.q_b": 8.21e-03, "node-nodrop-packed/L1.k_w": 6.63e-03, "node-nodrop-packed/L1.v_w": 3.43e-03,
    "node-nodrop-packed/L1.v_b": 3.40e-03, "node-nodrop-packed/L1.o_w": 4.72e-03, "node-nodrop-packed/L1.o_b": 3.17e-03, "node-nodrop-packed/L1.ln1_w": 5.50e-03,
    "node-nodrop-packed/L1.ln1_b": 3.05e-03, "node-nodrop-packed/L1.fc1_w": 4.24e-03, "node-nodrop-packed/L1.fc1_b": 3.47e-03,
    "node-nodrop-packed/L1.fc2_w": 2.91e-03, "node-nodrop-packed/L1.fc2_b": 1.52e-03, "node-nodrop-packed/L1.ln2_w": 3.78e-03,
    "node-nodrop-packed/L1.ln2_b": 0.00e+00,
    "node-preln-padded/hidden0": 2.67e-03, "node-preln-padded/hidden1": 5.02e-03, "node-preln-padded/dh_in": 1.24e-02, "node-preln-padded/L0.q_w": 6.42e-03,
    "node-preln-padded/L0.q_b": 4.22e-03, "node-preln-padded/L0.k_w": 7.32e-03, "node-preln-padded/L0.v_w": 3.67e-03, "node-preln-padded/L0.v_b": 3.49e-03,
    "node-preln-padded/L0.o_w": 4.14e-03, "node-preln-padded/L0.o_b": 3.23e-03, "node-preln-padded/L0.ln1_w": 5.41e-03, "node-preln-padded/L0.ln1_b": 4.02e-03,
    "node-preln-padded/L0.fc1_w": 3.74e-03, "node-preln-padded/L0.fc1_b": 2.78e-03, "node-preln-padded/L0.fc2_w": 4.42e-03, "node-preln-padded/L0.fc2_b": 2.84e-03,
    "node-preln-padded/L0.ln2_w": 4.20e-03, "node-preln-padded/L0.ln2_b": 3.57e-03, "node-preln-padded/L1.q_w": 4.90e-03, "node-preln-padded/L1.q_b": 6.91e-03,
    "node-preln-padded/L1.k_w": 7.16e-03, "node-preln-padded/L1.v_w": 2.31e-03, "node-preln-padded/L1.v_b": 2.73e-03, "node-preln-padded/L1.o_w": 3.30e-03,
    "node-preln-padded/L1.o_b": 2.83e-03, "node-preln-padded/L1.ln1_w": 8.75e-03, "node-preln-padded/L1.ln1_b": 3.31e-03, "node-preln-padded/L1.fc1_w": 3.53e-03,
    "node-preln-padded/L1.fc1_b": 2.89e-03, "node-preln-padded/L1.fc2_w": 2.61e-03, "node-preln-padded/L1.fc2_b": 0.00e+00, "node-preln-padded/L1.ln2_w": 4.55e-03,
    "node-preln-padded/L1.ln2_b": 3.33e-03,
    "node-preln-packed/hidden0": 2.67e-03, "node-preln-packed/hidden1": 5.02e-03, "node-preln-packed/dh_in": 1.16e-02, "node-preln-packed/L0.q_w": 6.68e-03,
    "node-preln-packed/L0.q_b": 6.04e-03, "node-preln-packed/L0.k_w": 7.61e-03, "node-preln-packed/L0.v_w": 4.52e-03, "node-preln-packed/L0.v_b": 4.15e-03,
    "node-preln-packed/L0.o_w": 4.19e-03, "node-preln-packed/L0.o_b": 3.91e-03, "node-preln-packed/L0.ln1_w": 5.47e-03, "node-preln-packed/L0.ln1_b": 4.38e-03,
    "node-preln-packed/L0.fc1_w": 4.03e-03, "node-preln-packed/L0.fc1_b": 2.83e-03, "node-preln-packed/L0.fc2_w": 3.85e-03, "node-preln-packed/L0.fc2_b": 2.75e-03,
    "node-preln-packed/L0.ln2_w": 4.47e-03, "node-preln-packed/L0.ln2_b": 4.04e-03, "node-preln-packed/L1.q_w": 5.99e-03, "node-preln-packed/L1.q_b": 6.52e-03,
    "node-preln-packed/L1.k_w": 6.60e-03, "node-preln-packed/L1.v_w": 3.43e-03, "node-preln-packed/L1.v_b": 3.18e-03, "node-preln-packed/L1.o_w": 3.35e-03,
    "node-preln-packed/L1.o_b": 2.42e-03, "node-preln-packed/L1.ln1_w": 5.89e-03, "node-preln-packed/L1.ln1_b": 2.96e-03, "node-preln-packed/L1.fc1_w": 3.61e-03,
    "node-preln-packed/L1.fc1_b": 3.06e-03, "node-preln-packed/L1.fc2_w": 2.68e-03, "node-preln-packed/L1.fc2_b": 0.00e+00, "node-preln-packed/L1.ln2_w": 3.62e-03,
    "node-preln-packed/L1.ln2_b": 3.04e-03,
    "node-preln-quickgelu/hidden0": 2.58e-03, "node-preln-quickgelu/hidden1": 3.29e-03, "node-preln-quickgelu/dh_in": 9.67e-03,
    "node-preln-quickgelu/L0.q_w": 6.03e-03, "node-preln-quickgelu/L0.q_b": 4.78e-03, "node-preln-quickgelu/L0.k_w": 6.23e-03,
    "node-preln-quickgelu/L0.v_w": 6.08e-03, "node-preln-quickgelu/L0.v_b": 3.50e-03, "node-preln-quickgelu/L0.o_w": 3.87e-03,
    "node-preln-quickgelu/L0.o_b": 2.89e-03, "node-preln-quickgelu/L0.ln1_w": 4.78e-03, "node-preln-quickgelu/L0.ln1_b": 4.06e-03,
    "node-preln-quickgelu/L0.fc1_w": 4.78e-03, "node-preln-quickgelu/L0.fc1_b": 4.21e-03, "node-preln-quickgelu/L0.fc2_w": 3.67e-03,
    "node-preln-quickgelu/L0.fc2_b": 2.26e-03, "node-preln-quickgelu/L0.ln2_w": 3.78e-03, "node-preln-quickgelu/L0.ln2_b": 3.43e-03,
    "node-preln-quickgelu/L1.q_w": 6.37e-03, "node-preln-quickgelu/L1.q_b": 4.93e-03, "node-preln-quickgelu/L1.k_w": 4.87e-03,
    "node-preln-quickgelu/L1.v_w": 3.51e-03, "node-preln-quickgelu/L1.v_b": 3.51e-03, "node-preln-quickgelu/L1.o_w": 3.78e-03,
    "node-preln-quickgelu/L1.o_b": 2.48e-03, "node-preln-quickgelu/L1.ln1_w": 4.56e-03, "node-preln-quickgelu/L1.ln1_b": 2.52e-03,
    "node-preln-quickgelu/L1.fc1_w": 2.89e-03, "node-preln-quickgelu/L1.fc1_b": 3.15e-03, "node-preln-quickgelu/L1.fc2_w": 2.63e-03,
    "node-preln-quickgelu/L1.fc2_b": 0.00e+00, "node-preln-quickgelu/L1.ln2_w": 5.07e-03, "node-preln-quickgelu/L1.ln2_b": 2.98e-03,
    "node-n3-mixed/hidden0": 9.42e-03, "node-n3-mixed/hidden1": 1.25e-02, "node-n3-mixed/hidden2": 1.11e-02, "node-n3-mixed/dh_in": 1.39e-02,
    "node-n3-mixed/L1.q_w": 8.67e-03, "node-n3-mixed/L1.q_b": 6.48e-03, "node-n3-mixed/L1.k_w": 1.01e-02, "node-n3-mixed/L1.v_w": 7.60e-03,
    "node-n3-mixed/L1.v_b": 6.06e-03, "node-n3-mixed/L1.o_w": 5.83e-03, "node-n3-mixed/L1.o_b": 5.31e-03, "node-n3-mixed/L1.ln1_w": 6.57e-03,
    "node-n3-mixed/L1.ln1_b": 5.70e-03, "node-n3-mixed/L1.fc1_w": 5.48e-03, "node-n3-mixed/L1.fc1_b": 4.85e-03, "node-n3-mixed/L1.fc2_w": 7.63e-03,
    "node-n3-mixed/L1.fc2_b": 3.41e-03, "node-n3-mixed/L1.ln2_w": 5.52e-03, "node-n3-mixed/L1.ln2_b": 4.67e-03,
    "node-preln-n3-mixed/hidden0": 2.67e-03, "node-preln-n3-mixed/hidden1": 3.34e-03, "node-preln-n3-mixed/hidden2": 4.12e-03,
    "node-preln-n3-mixed/dh_in": 1.04e-02, "node-preln-n3-mixed/L1.q_w": 6.77e-03, "node-preln-n3-mixed/L1.q_b": 4.99e-03, "node-preln-n3-mixed/L1.k_w": 6.09e-03,
    "node-preln-n3-mixed/L1.v_w": 3.57e-03, "node-preln-n3-mixed/L1.v_b": 3.21e-03, "node-preln-n3-mixed/L1.o_w": 4.04e-03, "node-preln-n3-mixed/L1.o_b": 3.74e-03,
    "node-preln-n3-mixed/L1.ln1_w": 4.50e-03, "node-preln-n3-mixed/L1.ln1_b": 4.66e-03, "node-preln-n3-mixed/L1.fc1_w": 4.32e-03,
    "node-preln-n3-mixed/L1.fc1_b": 3.69e-03, "node-preln-n3-mixed/L1.fc2_w": 3.49e-03, "node-preln-n3-mixed/L1.fc2_b": 3.11e-03,
    "node-preln-n3-mixed/L1.ln2_w": 5.64e-03, "node-preln-n3-mixed/L1.ln2_b": 4.88e-03,
    "wsum-plain/mixed": 3.66e-03, "wsum-plain/dh0": 3.68e-03, "wsum-plain/dh1": 3.20e-03, "wsum-plain/dh2": 3.73e-03, "wsum-plain/dh3": 3.46e-03,
    "wsum-normalize/mixed": 3.81e-03, "wsum-normalize/dh0": 5.24e-03, "wsum-normalize/dh1": 5.33e-03, "wsum-normalize/dh2": 6.24e-03,
    "wsum-normalize/dh3": 5.84e-03,
    "branch-hd64-n2-post-p0.1/out": 5.67e-03, "branch-hd64-n2-post-p0.1/dcls": 5.66e-03, "branch-hd64-n2-post-p0.1/dframes": 1.35e-02,
    "branch-hd64-n2-post-p0.1/L0.in_w": 8.82e-03, "branch-hd64-n2-post-p0.1/L0.in_b.q": 1.49e-02, "branch-hd64-n2-post-p0.1/L0.in_b.v": 4.71e-03,
    "branch-hd64-n2-post-p0.1/L0.out_w": 6.90e-03, "branch-hd64-n2-post-p0.1/L0.out_b": 4.99e-03, "branch-hd64-n2-post-p0.1/L0.n1_w": 6.58e-03,
    "branch-hd64-n2-post-p0.1/L0.n1_b": 4.59e-03, "branch-hd64-n2-post-p0.1/L0.l1_w": 5.17e-03, "branch-hd64-n2-post-p0.1/L0.l1_b": 3.50e-03,
    "branch-hd64-n2-post-p0.1/L0.l2_w": 6.72e-03, "branch-hd64-n2-post-p0.1/L0.l2_b": 4.05e-03, "branch-hd64-n2-post-p0.1/L0.n2_w": 6.37e-03,
    "branch-hd64-n2-post-p0.1/L0.n2_b": 2.68e-03, "branch-hd64-n2-post-p0.1/L1.in_w": 7.12e-03, "branch-hd64-n2-post-p0.1/L1.in_b.q": 1.19e-02,
    "branch-hd64-n2-post-p0.1/L1.in_b.v": 2.49e-03, "branch-hd64-n2-post-p0.1/L1.out_w": 1.37e-02, "branch-hd64-n2-post-p0.1/L1.out_b": 1.55e-03,
    "branch-hd64-n2-post-p0.1/L1.n1_w": 4.81e-03, "branch-hd64-n2-post-p0.1/L1.n1_b": 1.59e-03, "branch-hd64-n2-post-p0.1/L1.l1_w": 4.67e-03,
    "branch-hd64-n2-post-p0.1/L1.l1_b": 3.23e-03, "branch-hd64-n2-post-p0.1/L1.l2_w": 5.19e-03, "branch-hd64-n2-post-p0.1/L1.l2_b": 4.84e-04,
    "branch-hd64-n2-post-p0.1/L1.n2_w": 4.25e-03, "branch-hd64-n2-post-p0.1/L1.n2_b": 3.27e-04, "branch-hd64-n2-post-p0.1/nf_w": 3.92e-03,
    "branch-hd64-n2-post-p0.1/nf_b": 0.00e+00,
    "branch-hd96-n2-pre-p0.1/out": 3.11e-03, "branch-hd96-n2-pre-p0.1/dcls": 4.49e-03, "branch-hd96-n2-pre-p0.1/dframes": 1.07e-02,
    "branch-hd96-n2-pre-p0.1/L0.in_w": 4.79e-03, "branch-hd96-n2-pre-p0.1/L0.in_b.q": 4.73e-03, "branch-hd96-n2-pre-p0.1/L0.in_b.v": 4.25e-03,
    "branch-hd96-n2-pre-p0.1/L0.out_w": 8.01e-03, "branch-hd96-n2-pre-p0.1/L0.out_b": 2.59e-03, "branch-hd96-n2-pre-p0.1/L0.n1_w": 3.59e-03,
    "branch-hd96-n2-pre-p0.1/L0.n1_b": 2.68e-03, "branch-hd96-n2-pre-p0.1/L0.l1_w": 4.24e-03, "branch-hd96-n2-pre-p0.1/L0.l1_b": 3.52e-03,
    "branch-hd96-n2-pre-p0.1/L0.l2_w": 4.81e-03, "branch-hd96-n2-pre-p0.1/L0.l2_b": 2.75e-03, "branch-hd96-n2-pre-p0.1/L0.n2_w": 4.76e-03,
    "branch-hd96-n2-pre-p0.1/L0.n2_b": 3.16e-03, "branch-hd96-n2-pre-p0.1/L1.in_w": 4.10e-03, "branch-hd96-n2-pre-p0.1/L1.in_b.q": 7.05e-03,
    "branch-hd96-n2-pre-p0.1/L1.in_b.v": 1.71e-03, "branch-hd96-n2-pre-p0.1/L1.out_w": 4.82e-03, "branch-hd96-n2-pre-p0.1/L1.out_b": 6.69e-04,
    "branch-hd96-n2-pre-p0.1/L1.n1_w": 3.57e-03, "branch-hd96-n2-pre-p0.1/L1.n1_b": 2.57e-03, "branch-hd96-n2-pre-p0.1/L1.l1_w": 2.76e-03,
    "branch-hd96-n2-pre-p0.1/L1.l1_b": 2.03e-03, "branch-hd96-n2-pre-p0.1/L1.l2_w": 1.46e-03, "branch-hd96-n2-pre-p0.1/L1.l2_b": 4.65e-04,
    "branch-hd96-n2-pre-p0.1/L1.n2_w": 2.76e-03, "branch-hd96-n2-pre-p0.1/L1.n2_b": 1.36e-03, "branch-hd96-n2-pre-p0.1/nf_w": 1.88e-03,
    "branch-hd96-n2-pre-p0.1/nf_b": 0.00e+00,
    "branch-hd128-n2-post-p0/out": 8.07e-03, "branch-hd128-n2-post-p0/dcls": 4.45e-03, "branch-hd128-n2-post-p0/dframes": 1.44e-02,
    "branch-hd128-n2-post-p0/L0.in_w": 4.75e-03, "branch-hd128-n2-post-p0/L0.in_b.q": 6.92e-03, "branch-hd128-n2-post-p0/L0.in_b.v": 4.62e-03,
    "branch-hd128-n2-post-p0/L0.out_w": 8.12e-03, "branch-hd128-n2-post-p0/L0.out_b": 3.20e-03, "branch-hd128-n2-post-p0/L0.n1_w": 3.90e-03,
    "branch-hd128-n2-post-p0/L0.n1_b": 3.26e-03, "branch-hd128-n2-post-p0/L0.l1_w": 5.61e-03, "branch-hd128-n2-post-p0/L0.l1_b": 3.66e-03,
    "branch-hd128-n2-post-p0/L0.l2_w": 4.58e-03, "branch-hd128-n2-post-p0/L0.l2_b": 2.92e-03, "branch-hd128-n2-post-p0/L0.n2_w": 2.87e-03,
    "branch-hd128-n2-post-p0/L0.n2_b": 3.00e-03, "branch-hd128-n2-post-p0/L1.in_w": 8.67e-03, "branch-hd128-n2-post-p0/L1.in_b.q": 5.69e-03,
    "branch-hd128-n2-post-p0/L1.in_b.v": 2.61e-03, "branch-hd128-n2-post-p0/L1.out_w": 3.46e-03, "branch-hd128-n2-post-p0/L1.out_b": 1.07e-03,
    "branch-hd128-n2-post-p0/L1.n1_w": 2.53e-03, "branch-hd128-n2-post-p0/L1.n1_b": 1.05e-03, "branch-hd128-n2-post-p0/L1.l1_w": 4.77e-03,
    "branch-hd128-n2-post-p0/L1.l1_b": 2.76e-03, "branch-hd128-n2-post-p0/L1.l2_w": 2.74e-03, "branch-hd128-n2-post-p0/L1.l2_b": 3.71e-04,
    "branch-hd128-n2-post-p0/L1.n2_w": 2.92e-03, "branch-hd128-n2-post-p0/L1.n2_b": 3.39e-04, "branch-hd128-n2-post-p0/nf_w": 2.30e-03,
    "branch-hd128-n2-post-p0/nf_b": 0.00e+00,
    "branch-hd64-n1-pre-p0/out": 1.72e-03, "branch-hd64-n1-pre-p0/dcls": 2.89e-03, "branch-hd64-n1-pre-p0/dframes": 1.13e-02,
    "branch-hd64-n1-pre-p0/L0.in_w": 5.86e-03, "branch-hd64-n1-pre-p0/L0.in_b.q": 7.43e-03, "branch-hd64-n1-pre-p0/L0.in_b.v": 1.94e-03,
    "branch-hd64-n1-pre-p0/L0.out_w": 5.08e-03, "branch-hd64-n1-pre-p0/L0.out_b": 3.41e-04, "branch-hd64-n1-pre-p0/L0.n1_w": 4.95e-03,
    "branch-hd64-n1-pre-p0/L0.n1_b": 3.09e-03, "branch-hd64-n1-pre-p0/L0.l1_w": 1.95e-03, "branch-hd64-n1-pre-p0/L0.l1_b": 1.77e-03,
    "branch-hd64-n1-pre-p0/L0.l2_w": 9.18e-04, "branch-hd64-n1-pre-p0/L0.l2_b": 9.26e-05, "branch-hd64-n1-pre-p0/L0.n2_w": 1.02e-03,
    "branch-hd64-n1-pre-p0/L0.n2_b": 1.04e-03, "branch-hd64-n1-pre-p0/nf_w": 7.00e-04, "branch-hd64-n1-pre-p0/nf_b": 0.00e+00,
    "branch-hd64-n3-post-p0.1/out": 7.45e-03, "branch-hd64-n3-post-p0.1/dcls": 6.72e-03, "branch-hd64-n3-post-p0.1/dframes": 1.92e-02,
    "branch-hd64-n3-post-p0.1/L0.in_w": 5.40e-03, "branch-hd64-n3-post-p0.1/L0.in_b.q": 1.21e-02, "branch-hd64-n3-post-p0.1/L0.in_b.v": 4.43e-03,
    "branch-hd64-n3-post-p0.1/L0.out_w": 5.02e-03, "branch-hd64-n3-post-p0.1/L0.out_b": 4.51e-03, "branch-hd64-n3-post-p0.1/L0.n1_w": 6.09e-03,
    "branch-hd64-n3-post-p0.1/L0.n1_b": 3.12e-03, "branch-hd64-n3-post-p0.1/L0.l1_w": 8.79e-03, "branch-hd64-n3-post-p0.1/L0.l1_b": 5.19e-03,
    "branch-hd64-n3-post-p0.1/L0.l2_w": 9.66e-03, "branch-hd64-n3-post-p0.1/L0.l2_b": 5.41e-03, "branch-hd64-n3-post-p0.1/L0.n2_w": 1.40e-02,
    "branch-hd64-n3-post-p0.1/L0.n2_b": 4.32e-03, "branch-hd64-n3-post-p0.1/L1.in_w": 7.09e-03, "branch-hd64-n3-post-p0.1/L1.in_b.q": 6.86e-03,
    "branch-hd64-n3-post-p0.1/L1.in_b.v": 5.59e-03, "branch-hd64-n3-post-p0.1/L1.out_w": 8.56e-03, "branch-hd64-n3-post-p0.1/L1.out_b": 5.81e-03,
    "branch-hd64-n3-post-p0.1/L1.n1_w": 1.41e-02, "branch-hd64-n3-post-p0.1/L1.n1_b": 5.61e-03, "branch-hd64-n3-post-p0.1/L1.l1_w": 7.62e-03,
    "branch-hd64-n3-post-p0.1/L1.l1_b": 4.12e-03, "branch-hd64-n3-post-p0.1/L1.l2_w": 6.40e-03, "branch-hd64-n3-post-p0.1/L1.l2_b": 4.04e-03,
    "branch-hd64-n3-post-p0.1/L1.n2_w": 7.64e-03, "branch-hd64-n3-post-p0.1/L1.n2_b": 2.57e-03, "branch-hd64-n3-post-p0.1/L2.in_w": 4.47e-03,
    "branch-hd64-n3-post-p0.1/L2.in_b.q": 1.06e-02, "branch-hd64-n3-post-p0.1/L2.in_b.v": 2.47e-03, "branch-hd64-n3-post-p0.1/L2.out_w": 7.67e-03,
    "branch-hd64-n3-post-p0.1/L2.out_b": 2.15e-03, "branch-hd64-n3-post-p0.1/L2.n1_w": 6.75e-03, "branch-hd64-n3-post-p0.1/L2.n1_b": 2.55e-03,
    "branch-hd64-n3-post-p0.1/L2.l1_w": 5.60e-03, "branch-hd64-n3-post-p0.1/L2.l1_b": 4.53e-03, "branch-hd64-n3-post-p0.1/L2.l2_w": 4.92e-03,
    "branch-hd64-n3-post-p0.1/L2.l2_b": 1.13e-03, "branch-hd64-n3-post-p0.1/L2.n2_w": 6.38e-03, "branch-hd64-n3-post-p0.1/L2.n2_b": 6.95e-04,
    "branch-hd64-n3-post-p0.1/nf_w": 4.89e-03, "branch-hd64-n3-post-p0.1/nf_b": 0.00e+00,
    "branch-hd64-n3-pre-p0/out": 3.17e-03, "branch-hd64-n3-pre-p0/dcls": 3.84e-03, "branch-hd64-n3-pre-p0/dframes": 1.28e-02,
    "branch-hd64-n3-pre-p0/L0.in_w": 5.19e-03, "branch-hd64-n3-pre-p0/L0.in_b.q": 4.44e-03, "branch-hd64-n3-pre-p0/L0.in_b.v": 4.22e-03,
    "branch-hd64-n3-pre-p0/L0.out_w": 6.15e-03, "branch-hd64-n3-pre-p0/L0.out_b": 4.52e-03, "branch-hd64-n3-pre-p0/L0.n1_w": 3.53e-03,
    "branch-hd64-n3-pre-p0/L0.n1_b": 5.26e-03, "branch-hd64-n3-pre-p0/L0.l1_w": 4.00e-03, "branch-hd64-n3-pre-p0/L0.l1_b": 4.28e-03,
    "branch-hd64-n3-pre-p0/L0.l2_w": 4.92e-03, "branch-hd64-n3-pre-p0/L0.l2_b": 2.63e-03, "branch-hd64-n3-pre-p0/L0.n2_w": 5.55e-03,
    "branch-hd64-n3-pre-p0/L0.n2_b": 4.36e-03, "branch-hd64-n3-pre-p0/L1.in_w": 4.08e-03, "branch-hd64-n3-pre-p0/L1.in_b.q": 4.55e-03,
    "branch-hd64-n3-pre-p0/L1.in_b.v": 2.78e-03, "branch-hd64-n3-pre-p0/L1.out_w": 8.33e-03, "branch-hd64-n3-pre-p0/L1.out_b": 2.52e-03,
    "branch-hd64-n3-pre-p0/L1.n1_w": 4.91e-03, "branch-hd64-n3-pre-p0/L1.n1_b": 2.25e-03, "branch-hd64-n3-pre-p0/L1.l1_w": 3.29e-03,
    "branch-hd64-n3-pre-p0/L1.l1_b": 3.44e-03, "branch-hd64-n3-pre-p0/L1.l2_w": 3.51e-03, "branch-hd64-n3-pre-p0/L1.l2_b": 1.85e-03,
    "branch-hd64-n3-pre-p0/L1.n2_w": 2.77e-03, "branch-hd64-n3-pre-p0/L1.n2_b": 2.29e-03, "branch-hd64-n3-pre-p0/L2.in_w": 3.62e-03,
    "branch-hd64-n3-pre-p0/L2.in_b.q": 6.65e-03, "branch-hd64-n3-pre-p0/L2.in_b.v": 1.96e-03, "branch-hd64-n3-pre-p0/L2.out_w": 3.48e-03,
    "branch-hd64-n3-pre-p0/L2.out_b": 4.65e-04, "branch-hd64-n3-pre-p0/L2.n1_w": 2.34e-03, "branch-hd64-n3-pre-p0/L2.n1_b": 2.17e-03,
    "branch-hd64-n3-pre-p0/L2.l1_w": 1.45e-03, "branch-hd64-n3-pre-p0/L2.l1_b": 1.45e-03, "branch-hd64-n3-pre-p0/L2.l2_w": 1.29e-03,
    "branch-hd64-n3-pre-p0/L2.l2_b": 3.77e-04, "branch-hd64-n3-pre-p0/L2.n2_w": 2.73e-03, "branch-hd64-n3-pre-p0/L2.n2_b": 1.13e-03,
    "branch-hd64-n3-pre-p0/nf_w": 1.41e-03, "branch-hd64-n3-pre-p0/nf_b": 0.00e+00,
    "tower-T17/feat": 3.79e-03, "tower-T17/class_embedding": 4.64e-03, "tower-T17/positional_embedding": 4.64e-03, "tower-T17/proj": 2.11e-03,
    "tower-T17/conv1.weight": 8.57e-03, "tower-T17/ln_pre.weight": 6.74e-03, "tower-T17/ln_pre.bias": 6.25e-03,
    "tower-T17/transformer.resblocks.0.attn.in_proj_weight": 1.09e-02, "tower-T17/transformer.resblocks.0.attn.in_proj_bias.q": 7.93e-03,
    "tower-T17/transformer.resblocks.0.attn.in_proj_bias.v": 6.73e-03, "tower-T17/transformer.resblocks.0.attn.out_proj.weight": 9.61e-03,
    "tower-T17/transformer.resblocks.0.attn.out_proj.bias": 7.19e-03, "tower-T17/transformer.resblocks.0.ln_1.weight": 8.97e-03,
    "tower-T17/transformer.resblocks.0.ln_1.bias": 6.27e-03, "tower-T17/transformer.resblocks.0.mlp.c_fc.weight": 6.17e-03,
    "tower-T17/transformer.resblocks.0.mlp.c_fc.bias": 5.14e-03, "tower-T17/transformer.resblocks.0.mlp.c_proj.weight": 8.27e-03,
    "tower-T17/transformer.resblocks.0.mlp.c_proj.bias": 7.34e-03, "tower-T17/transformer.resblocks.0.ln_2.weight": 9.19e-03,
    "tower-T17/transformer.resblocks.0.ln_2.bias": 7.03e-03, "tower-T17/transformer.resblocks.1.attn.in_proj_weight": 6.28e-03,
    "tower-T17/transformer.resblocks.1.attn.in_proj_bias.q": 1.12e-02, "tower-T17/transformer.resblocks.1.attn.in_proj_bias.v": 3.80e-03,
    "tower-T17/transformer.resblocks.1.attn.out_proj.weight": 8.96e-03, "tower-T17/transformer.resblocks.1.attn.out_proj.bias": 4.98e-03,
    "tower-T17/transformer.resblocks.1.ln_1.weight": 9.14e-03, "tower-T17/transformer.resblocks.1.ln_1.bias": 5.16e-03,
    "tower-T17/transformer.resblocks.1.mlp.c_fc.weight": 3.34e-03, "tower-T17/transformer.resblocks.1.mlp.c_fc.bias": 3.28e-03,
    "tower-T17/transformer.resblocks.1.mlp.c_proj.weight": 3.65e-03, "tower-T17/transformer.resblocks.1.mlp.c_proj.bias": 2.10e-03,
    "tower-T17/transformer.resblocks.1.ln_2.weight": 5.22e-03, "tower-T17/transformer.resblocks.1.ln_2.bias": 3.69e-03, "tower-T17/ln_post.weight": 2.94e-03,
    "tower-T17/ln_post.bias": 0.00e+00,
    "tower-T65/feat": 3.41e-03, "tower-T65/class_embedding": 3.27e-03, "tower-T65/positional_embedding": 3.27e-03, "tower-T65/proj": 1.89e-03,
    "tower-T65/conv1.weight": 8.76e-03, "tower-T65/ln_pre.weight": 2.92e-03, "tower-T65/ln_pre.bias": 4.36e-03,
    "tower-T65/transformer.resblocks.0.attn.in_proj_weight": 7.37e-03, "tower-T65/transformer.resblocks.0.attn.in_proj_bias.q": 1.04e-02,
    "tower-T65/transformer.resblocks.0.attn.in_proj_bias.v": 4.40e-03, "tower-T65/transformer.resblocks.0.attn.out_proj.weight": 4.45e-03,
    "tower-T65/transformer.resblocks.0.attn.out_proj.bias": 3.61e-03, "tower-T65/transformer.resblocks.0.ln_1.weight": 7.60e-03,
    "tower-T65/transformer.resblocks.0.ln_1.bias": 6.15e-03, "tower-T65/transformer.resblocks.0.mlp.c_fc.weight": 3.51e-03,
    "tower-T65/transformer.resblocks.0.mlp.c_fc.bias": 3.62e-03, "tower-T65/transformer.resblocks.0.mlp.c_proj.weight": 2.73e-03,
    "tower-T65/transformer.resblocks.0.mlp.c_proj.bias": 2.17e-03, "tower-T65/transformer.resblocks.0.ln_2.weight": 6.56e-03,
    "tower-T65/transformer.resblocks.0.ln_2.bias": 5.30e-03, "tower-T65/transformer.resblocks.1.attn.in_proj_weight": 4.85e-03,
    "tower-T65/transformer.resblocks.1.attn.in_proj_bias.q": 7.80e-03, "tower-T65/transformer.resblocks.1.attn.in_proj_bias.v": 3.17e-03,
    "tower-T65/transformer.resblocks.1.attn.out_proj.weight": 2.74e-03, "tower-T65/transformer.resblocks.1.attn.out_proj.bias": 1.73e-03,
    "tower-T65/transformer.resblocks.1.ln_1.weight": 3.10e-03, "tower-T65/transformer.resblocks.1.ln_1.bias": 4.30e-03,
    "tower-T65/transformer.resblocks.1.mlp.c_fc.weight": 3.69e-03, "tower-T65/transformer.resblocks.1.mlp.c_fc.bias": 2.87e-03,
    "tower-T65/transformer.resblocks.1.mlp.c_proj.weight": 2.78e-03, "tower-T65/transformer.resblocks.1.mlp.c_proj.bias": 1.50e-03,
    "tower-T65/transformer.resblocks.1.ln_2.weight": 3.36e-03, "tower-T65/transformer.resblocks.1.ln_2.bias": 4.05e-03, "tower-T65/ln_post.weight": 1.58e-03,
    "tower-T65/ln_post.bias": 0.00e+00,
}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    """values a bf16 tensor can hold, as fp32"""
    return t.to(BF).float()


class Judge:
    """Counts what it judged; prints key / worst / model / bound per tensor."""

    def __init__(self):
        self.rows = self.tensors = self.zero_slices = 0

    def check(self, key, kind, got, ref):
        assert got.shape == ref.shape and got.numel() > 0, (key, got.shape, ref.shape)
        assert torch.isfinite(got.double()).all(), key
        bound = R.bound_of(MODEL[key])
        if kind == "rows":
            m = R.row_metric(got.double().cpu(), ref)
            worst = m.max().item()
            self.rows += m.numel()
            print(f"{key:52s} worst row {worst:.3e}  model {MODEL[key]:.2e}  bound {bound:.3e}  rows {m.numel()}")
            assert worst <= bound, (key, "row", int(m.flatten().argmax()), "of", m.numel(), "metric", worst, "bound", bound)
        else:
            worst = R.tensor_metric(got.double().cpu(), ref)
            self.tensors += 1
            print(f"{key:52s} tensor    {worst:.3e}  model {MODEL[key]:.2e}  bound {bound:.3e}")
            assert worst <= bound, (key, "metric", worst, "bound", bound)

    def zero_slice(self, key, k_slice, q_slice):
        """an analytically zero k-bias slice: the rule of tests/test_dropout_gpu.py"""
        kn, qn = k_slice.float().norm().item(), q_slice.float().norm().item()
        self.zero_slices += 1
        print(f"{key:52s} zero      |k| {kn:.3e}  |q| {qn:.3e}")
        assert kn < 1e-2 * qn, (key, kn, qn)

    def all(self, cid, got, ref):
        """got / ref: name -> (kind, tensor) from the family's `*_tensors`; "zero" entries hold (k slice, q slice)."""
        assert list(got) == list(ref), (sorted(set(got) ^ set(ref)))
        for name, (kind, r) in ref.items():
            if kind == "zero":
                self.zero_slice(f"{cid}/{name}", *got[name][1])
            else:
                self.check(f"{cid}/{name}", kind, got[name][1], r)


def _split3(prefix, t, out):
    """The q | k | v bias gradient [3D]: q and v judged as tensors, k by the zero rule."""
    D = t.shape[0] // 3
    out[prefix + ".q"] = ("tensor", t[:D])
    out[prefix + ".k"] = ("zero", (t[D:2 * D], t[:D]))
    out[prefix + ".v"] = ("tensor", t[2 * D:])


# ================================================================================================ a. the layer node
@dataclasses.dataclass(frozen=True)
class NodeCase:
    id: str
    rows: tuple               # rows per utterance in the layout
    lens: tuple               # valid keys per utterance
    packed: bool
    train: tuple              # one flag per layer
    pre_ln: bool = False
    drop: bool = False
    act: str = "gelu"

    @property
    def B(self):
        return len(self.rows)

    @property
    def n(self):
        return len(self.train)

    @property
    def offsets(self):
        off = [0]
        for r in self.rows:
            off.append(off[-1] + r)
        return off


_PAD, _PACK = ((70, 70, 70), (70, 64, 33)), ((70, 65, 2, 1), (70, 65, 2, 1))
NODE_CASES = (NodeCase("node-nodrop-padded", *_PAD, False, (True, True)), NodeCase("node-nodrop-packed", *_PACK, True, (True, True)),
              NodeCase("node-preln-padded", *_PAD, False, (True, True), pre_ln=True), NodeCase("node-preln-packed", *_PACK, True, (True, True), pre_ln=True),
              NodeCase("node-preln-quickgelu", (70, 70, 70), (70, 70, 70), False, (True, True), pre_ln=True, act="quickgelu"),
              NodeCase("node-n3-mixed", *_PAD, False, (False, True, False), drop=True), NodeCase("node-preln-n3-mixed", *_PAD, False, (False, True, False), pre_ln=True))
NODE_D, NODE_H, NODE_FFN = 128, 2, 256
NODE_RATES = dict(hidden=0.1, attention=0.1, activation=0.1)
NODE_SEED = 424242


def node_case(cid):
    return next(c for c in NODE_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def node_inputs(cid):
    """16 tensors per layer (matrices hold bf16 values: the 16-bit operand copy is exact; 0.08 randn at d = 128 makes each branch as large as the residual it joins,
    see _tiny_hubert of test_train_mode_parity_gpu.py), h_in and the gradient of every hidden state (bf16 values, non-zero on valid rows, zero on rows >= lens[b])."""
    c = node_case(cid)
    d, ffn = NODE_D, NODE_FFN
    g = _g(700 + len(cid) + 10 * c.n)
    shapes = [(d, d), (d,), (d, d), (d,), (d, d), (d,), (d, d), (d,), (d,), (d,), (ffn, d), (ffn,), (d, ffn), (d,), (d,), (d,)]
    layers = []
    for _ in range(c.n):
        ps = []
        for i, sh in enumerate(shapes):
            t = _bf(0.08 * torch.randn(*sh, generator=g)) if len(sh) == 2 else 0.05 * torch.randn(*sh, generator=g)
            ps.append(1.0 + t if i in (8, 14) else t)
        layers.append(ps)
    M = c.offsets[-1]
    h_in = _bf(torch.randn(M, d, generator=g))
    dh = _bf(torch.randn(c.n, M, d, generator=g))
    for b, n in enumerate(c.lens):
        dh[:, c.offsets[b] + n:c.offsets[b + 1]] = 0
    return dict(layers=layers, h_in=h_in, dh=dh)


def node_masks(c):
    if not c.drop:
        return [[None] * c.B for _ in range(c.n)]
    seeds = R.site_seeds(NODE_SEED, 4 * c.n)
    lay = dict(row_off=c.offsets, Tmax=max(c.rows)) if c.packed else dict(B=c.B, Tp=c.rows[0])
    return [[R.layer_masks(seeds[4 * li:4 * li + 4], lay, b, c.rows[b], NODE_D, NODE_FFN, NODE_H, NODE_RATES) for b in range(c.B)] for li in range(c.n)]


def node_reference(cid, model=False, wiring=(), train=None, swap_kv=False):
    """MUTANTS: wiring (train_mode_ref.layer_node and the bodies), train (other frozen / trained flags), swap_kv (k and v gradients exchanged)."""
    c, d = node_case(cid), node_inputs(cid)
    off = c.offsets
    xs = [d["h_in"][off[b]:off[b + 1]].double() for b in range(c.B)]
    dh = [[d["dh"][li, off[b]:off[b + 1]].double() for b in range(c.B)] for li in range(c.n)]
    layers = [[p.double() for p in lp] for lp in d["layers"]]
    res = R.layer_node(xs, layers, list(c.lens), node_masks(c), dh, c.train if train is None else train, model, wiring=wiring, pre_ln=c.pre_ln, act=c.act)
    if swap_kv:
        for gl in res["grads"]:
            if gl is not None:
                gl[2], gl[3], gl[4], gl[5] = gl[4], gl[5], gl[2], gl[3]
    return res


@functools.lru_cache(maxsize=None)
def node_reference_cached(cid):
    return node_reference(cid)


def node_tensors(c, res):
    """res: dict(hidden[li][b], dh_in[b], grads[li]) -> the judged tensors; a layer without gradients contributes none (the test asserts which)."""
    rows = lambda per: torch.cat([t[:n] for t, n in zip(per, c.lens)])      # noqa: E731
    out = {f"hidden{li}": ("rows", rows(res["hidden"][li])) for li in range(c.n)}
    out["dh_in"] = ("rows", rows(res["dh_in"]))
    for li in range(c.n):
        if res["grads"][li] is not None:
            for name, g in zip(R.LAYER_NAMES, res["grads"][li]):
                out[f"L{li}.{name}"] = ("zero", (g, res["grads"][li][1])) if name == "k_b" else ("tensor", g)
    return out


def _run_vit_bodies(c, params, h_in, dh):
    """The pre-LN body functions with the image tower's pair (QuickGELU, ops.attention without a key mask, the fused head-dim-64 backward), chained as
    HubertLayersTrainFn chains them -- that node takes no activation argument, train_vit.py calls the bodies the same way."""
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import ACT_QUICKGELU_PAIR, _f32, _layer_bwd_pre_ln, _layer_fwd_pre_ln, _param_grads, _w16
    from speechclip_amd.train_vit import ATTN_VIT
    shape = (c.B, c.rows[0], NODE_H, 1e-5)
    hidden = torch.empty(c.n, *h_in.shape, device=h_in.device, dtype=torch.float32)
    saved, h = [], h_in.float().contiguous()
    for li in range(c.n):
        qw, qb, kw, kb, vw, vb, *rest = params[16 * li:16 * li + 16]
        saved.append(_layer_fwd_pre_ln(h, _w16(torch.cat([qw, kw, vw], 0)), _f32(torch.cat([qb, kb, vb], 0)), rest, None, shape, None, hidden[li], None, (),
                                       attn=ATTN_VIT, act=ACT_QUICKGELU_PAIR))
        h = hidden[li]
    dh = dh.to(BF).contiguous()
    grads = [None] * len(params)
    g = dh[c.n - 1].clone()
    for li in range(c.n - 1, -1, -1):
        g, pieces = _layer_bwd_pre_ln(g, saved[li], params[16 * li:16 * li + 16], None, shape, None, True, None, (0, 0, 0, 0), attn=ATTN_VIT, act=ACT_QUICKGELU_PAIR)
        _param_grads(grads, 16 * li, *pieces)
        if li > 0:
            ops.axpy_bf16(g, dh[li - 1], 1.0)
    return hidden, g.float(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in NODE_CASES])
def test_layer_node_bodies_flags_and_depth_against_fp64(cid):
    from speechclip_amd.train_hubert import HubertLayersTrainFn
    c, d = node_case(cid), node_inputs(cid)
    ref = node_tensors(c, node_reference_cached(cid))
    dev = torch.device("cuda")
    off, M = c.offsets, c.offsets[-1]
    params = [p.clone().to(dev).requires_grad_(True) for lp in d["layers"] for p in lp]
    h_in = (d["h_in"] if c.pre_ln else d["h_in"].to(BF)).to(dev).requires_grad_(True)
    dh = (d["dh"] if c.pre_ln else d["dh"].to(BF)).to(dev)
    if c.act == "quickgelu":
        with torch.no_grad():
            hidden, dh_in, grads = _run_vit_bodies(c, [p.detach() for p in params], h_in.detach(), dh)
    else:
        meta = dict(B=c.B, Tp=max(c.rows), H=NODE_H, eps=1e-5, train=list(c.train), pre_ln=c.pre_ln)
        if c.drop:
            meta["drop"] = dict(NODE_RATES, seed=NODE_SEED)
        if c.packed:
            meta["pack"] = dict(row_off=off, rows_max=max(c.rows), total=M)
        hidden = HubertLayersTrainFn.apply(meta, h_in, torch.tensor(c.lens, dtype=torch.int32, device=dev), *params)
        hidden.backward(dh)
        dh_in, grads = h_in.grad, [p.grad for p in params]
        hidden = hidden.detach()
    torch.cuda.synchronize()
    assert hidden.shape == (c.n, M, NODE_D) and hidden.dtype == (torch.float32 if c.pre_ln else BF)
    split = lambda t: [t[off[b]:off[b + 1]].float().cpu() for b in range(c.B)]      # noqa: E731
    for b, n in enumerate(c.lens):
        assert not bool(dh_in[off[b] + n:off[b + 1]].any()), (b, "dh_in beyond the valid rows")
    got = dict(hidden=[split(hidden[li]) for li in range(c.n)], dh_in=split(dh_in), grads=[])
    for li in range(c.n):
        mine = grads[16 * li:16 * li + 16]
        if not c.train[li]:
            assert all(g is None for g in mine), "an untrained layer has no parameter gradients"
        got["grads"].append([g.float().cpu() for g in mine] if c.train[li] else None)
    J = Judge()
    J.all(cid, node_tensors(c, got), ref)
    trained = sum(c.train)
    assert (J.rows, J.tensors, J.zero_slices) == ((c.n + 1) * sum(c.lens), 15 * trained, trained)


# ================================================================================================ b. the layer mix
WSUM_N, WSUM_M, WSUM_D = 4, 137, 128
WSUM_W = (2.0, 0.25, -3.0, 0.5)          # one dominant weight, one near -3 (softmax 0.4 %)
WSUM_CASES = ("wsum-plain", "wsum-normalize")


@functools.lru_cache(maxsize=None)
def wsum_inputs():
    g = _g(811)
    hid = _bf(torch.randn(WSUM_N, WSUM_M, WSUM_D, generator=g) * 1.5 + 0.2)
    dm = _bf(8.0 * torch.randn(WSUM_M, WSUM_D, generator=g))       # large enough that the state with the 0.4 % weight still receives rows above the floor
    return dict(hid=hid, w=torch.tensor(WSUM_W), dm=dm)


def wsum_reference(cid, model=False, wiring=()):
    d = wsum_inputs()
    return N.weighted_sum_node(d["hid"].double(), d["w"].double(), cid == "wsum-normalize", d["dm"].double(), model, wiring)


@functools.lru_cache(maxsize=None)
def wsum_reference_cached(cid):
    return wsum_reference(cid)


def wsum_tensors(res):
    out = dict(mixed=("rows", res["mixed"]))
    out.update({f"dh{l}": ("rows", res["dhidden"][l]) for l in range(WSUM_N)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", WSUM_CASES)
def test_layer_mix_node_against_fp64(cid):
    from speechclip_amd.train_hubert import WeightedSumTrainFn
    d = wsum_inputs()
    dev = torch.device("cuda")
    hid = d["hid"].to(BF).to(dev).requires_grad_(True)
    mixed = WeightedSumTrainFn.apply(hid, d["w"].to(dev), cid == "wsum-normalize")
    mixed.backward(d["dm"].to(BF).to(dev))
    torch.cuda.synchronize()
    assert mixed.dtype == BF and hid.grad.shape == hid.shape
    J = Judge()
    J.all(cid, wsum_tensors(dict(mixed=mixed.detach().float().cpu(), dhidden=hid.grad.float().cpu())), wsum_tensors(wsum_reference_cached(cid)))
    assert (J.rows, J.tensors, J.zero_slices) == ((WSUM_N + 1) * WSUM_M, 0, 0)


# ================================================================================================ c. the branch stack
@dataclasses.dataclass(frozen=True)
class BranchCase:
    id: str
    D: int
    H: int
    n: int
    pre_ln: bool
    p: float
    draw: int = 0             # which draw of the random inputs (see BRANCH_CASES)

    @property
    def ffn(self):
        return 2 * self.D


# a cross, not the full product: each head dim (64 / 96 / 128) once with two layers; one and three layers at head dim 64; both norms with dropout and both without
BRANCH_CASES = (BranchCase("branch-hd64-n2-post-p0.1", 128, 2, 2, False, 0.1), BranchCase("branch-hd96-n2-pre-p0.1", 192, 2, 2, True, 0.1),
                BranchCase("branch-hd128-n2-post-p0", 256, 2, 2, False, 0.0), BranchCase("branch-hd64-n1-pre-p0", 128, 2, 1, True, 0.0),
                BranchCase("branch-hd64-n3-post-p0.1", 128, 2, 3, False, 0.1), BranchCase("branch-hd64-n3-pre-p0", 128, 2, 3, True, 0.0, draw=1))
# draw = 1: with the first draw of this case the k-bias slice of the last layer came to 1.2e-2 of the q slice's norm in the CPU MODEL itself (1.1e-2 on the MI355X):
# that gradient sums one query per (utterance, head), B H = 8 rounding terms, and the zero rule was ill-posed there (tools/train_node_bounds.py checks it now)
BRANCH_T, BRANCH_LEN = 69, (69, 63, 64, 1)          # key counts 70, 64, 65, 2: both sides of the 64-key tile edge and the shortest utterance
BRANCH_SEED = 31337
BRANCH_DOUT = 8.0          # scale of the output gradient: every frame row of the 70-key utterance (probabilities near 1 / 70) stays above the floor


def branch_case(cid):
    return next(c for c in BRANCH_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def branch_inputs(cid):
    """12 tensors per layer and the final norm (matrices hold bf16 values, std 0.9 / sqrt(fan_in): each branch as large as the residual it joins), the CLS token and
    the frames (bf16 values, zero beyond the length), the gradient of the output."""
    c = branch_case(cid)
    D, ffn, B = c.D, c.ffn, len(BRANCH_LEN)
    g = _g(900 + c.D + 10 * c.n + int(c.pre_ln) + 1000 * c.draw)
    mat = lambda o, i: _bf(0.9 * i ** -0.5 * torch.randn(o, i, generator=g))      # noqa: E731
    vec = lambda k: 0.05 * torch.randn(k, generator=g)                            # noqa: E731
    params = []
    for _ in range(c.n):
        params += [mat(3 * D, D), vec(3 * D), mat(D, D), vec(D), 1.0 + vec(D), vec(D), mat(ffn, D), vec(ffn), mat(D, ffn), vec(D), 1.0 + vec(D), vec(D)]
    params += [1.0 + vec(D), vec(D)]
    frames = _bf(torch.randn(B, BRANCH_T, D, generator=g))
    for b, l in enumerate(BRANCH_LEN):
        frames[b, l:] = 0
    return dict(params=params, cls=_bf(torch.randn(D, generator=g)), frames=frames, dout=BRANCH_DOUT * torch.randn(B, D, generator=g))


def branch_masks(c, reuse_last=None):
    B, Lq = len(BRANCH_LEN), BRANCH_T + 1
    return N.branch_masks(R.site_seeds(BRANCH_SEED, 4 * c.n), B, Lq, [l + 1 for l in BRANCH_LEN], c.D, c.ffn, c.H, c.p, reuse_last)


def branch_reference(cid, model=False, wiring=(), reuse_last=None, swap_kv=None):
    """MUTANTS: wiring (train_nodes_ref.branch_stack_node), reuse_last (a last-layer dropout site on the previous site's seed), swap_kv = layer: the k and v
    slices of that layer's in_proj gradients exchanged."""
    c, d = branch_case(cid), branch_inputs(cid)
    res = N.branch_stack_node(d["cls"].double(), [f.double() for f in d["frames"]], BRANCH_LEN, [p.double() for p in d["params"]], c.H, c.pre_ln,
                              branch_masks(c, reuse_last), d["dout"].double(), model, wiring=wiring)
    if swap_kv is not None:
        D = c.D
        for i in (12 * swap_kv, 12 * swap_kv + 1):
            t = res["grads"][i]
            res["grads"][i] = torch.cat([t[:D], t[2 * D:], t[D:2 * D]], 0)
    return res


@functools.lru_cache(maxsize=None)
def branch_reference_cached(cid):
    return branch_reference(cid)


def branch_tensors(c, res):
    """res: dict(out [B, D], dcls [D], dframes[b] (at least the valid rows), grads) -> the judged tensors"""
    out = dict(out=("rows", res["out"]), dcls=("tensor", res["dcls"].reshape(-1)),
               dframes=("rows", torch.cat([res["dframes"][b][:l] for b, l in enumerate(BRANCH_LEN)])))
    for li in range(c.n):
        for name, g in zip(N.BRANCH_NAMES, res["grads"][12 * li:12 * li + 12]):
            if name == "in_b":
                _split3(f"L{li}.in_b", g, out)
            else:
                out[f"L{li}.{name}"] = ("tensor", g)
    out["nf_w"], out["nf_b"] = ("tensor", res["grads"][-2]), ("tensor", res["grads"][-1])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in BRANCH_CASES])
def test_branch_stack_node_against_fp64(cid):
    from speechclip_amd.train_branch import BranchStackTrainFn
    c, d = branch_case(cid), branch_inputs(cid)
    dev = torch.device("cuda")
    params = [p.clone().to(dev).requires_grad_(True) for p in d["params"]]
    cls = d["cls"].view(1, 1, c.D).to(dev).requires_grad_(True)
    frames = d["frames"].to(BF).to(dev).requires_grad_(True)
    meta = dict(heads=c.H, eps=1e-5, pre_ln=c.pre_ln, drop_p=c.p, seed=BRANCH_SEED)
    out = BranchStackTrainFn.apply(meta, cls, frames, torch.tensor(BRANCH_LEN, dtype=torch.int32, device=dev), *params)
    out.backward(d["dout"].to(dev))
    torch.cuda.synchronize()
    assert out.shape == (len(BRANCH_LEN), c.D) and out.dtype == torch.float32 and frames.grad.shape == frames.shape
    df = frames.grad.float().cpu()
    for b, l in enumerate(BRANCH_LEN):
        assert not bool(df[b, l:].any()), (b, "dframes beyond the valid frames must be exactly zero")
    got = dict(out=out.detach().cpu(), dcls=cls.grad.float().cpu(), dframes=list(df), grads=[p.grad.float().cpu() for p in params])
    J = Judge()
    J.all(cid, branch_tensors(c, got), branch_tensors(c, branch_reference_cached(cid)))
    assert (J.rows, J.tensors, J.zero_slices) == (len(BRANCH_LEN) + sum(BRANCH_LEN), 1 + 13 * c.n + 2, c.n)


# ================================================================================================ d. the image tower
TOWER_CASES = ("tower-T17", "tower-T65")
TOWER_B = 3


@functools.lru_cache(maxsize=None)
def tower_setup(cid):
    """(ClipModel on the CPU, its fp64 oracle twin, image [3, 3, R, R], w fp64 [3, E], cfg of train_nodes_ref.image_tower_node)"""
    import vit_train_ref as V
    name = cid.split("-")[1]
    model, ref, image, w = V.make_tower(name)
    vis = model.model.visual
    cfg = dict(patch=V.TOWERS[name][1], heads=vis.transformer.heads, layers=len(vis.transformer.resblocks), eps=1e-5)
    return model, ref, image[:TOWER_B].contiguous(), w[:TOWER_B].contiguous(), cfg


def tower_reference(cid, model=False, wiring=(), swap_kv=False):
    """MUTANTS: wiring (train_nodes_ref.image_tower_node), swap_kv (the k and v slices of every in_proj gradient exchanged)."""
    _, ref, image, w, cfg = tower_setup(cid)
    params = {k: p.detach().double() for k, p in ref.visual.named_parameters()}
    res = N.image_tower_node(image.double(), params, cfg, w, model, wiring)
    if swap_kv:
        for k, t in res["grads"].items():
            if "in_proj" in k:
                D = t.shape[0] // 3
                res["grads"][k] = torch.cat([t[:D], t[2 * D:], t[D:2 * D]], 0)
    return res


@functools.lru_cache(maxsize=None)
def tower_reference_cached(cid):
    return tower_reference(cid)


def tower_tensors(res):
    out = dict(feat=("rows", res["feat"]))
    for k, g in res["grads"].items():
        if k.endswith("in_proj_bias"):
            _split3(k, g, out)
        else:
            out[k] = ("tensor", g)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", TOWER_CASES)
def test_image_tower_node_against_fp64(cid):
    import copy
    from speechclip_amd.train_vit import encode_image_train
    model, _, image, w, _ = tower_setup(cid)
    clip = copy.deepcopy(model.model).cuda()
    feat = encode_image_train(clip, image.cuda())
    (feat * w.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    vis = clip.visual
    grads = {k: p.grad.float().cpu() for k, p in vis.named_parameters()}
    assert len(grads) == 32
    dcls, dpos = vis.class_embedding.grad, vis.positional_embedding.grad
    assert torch.equal(dcls, dpos[0]) and dcls.data_ptr() != dpos.data_ptr(), "class_embedding.grad is row 0 of positional_embedding.grad, in a buffer of its own"
    ref = tower_reference_cached(cid)
    J = Judge()
    J.all(cid, tower_tensors(dict(feat=feat.detach().cpu(), grads={k: grads[k] for k in ref["grads"]})), tower_tensors(ref))
    nblk = len(vis.transformer.resblocks)
    assert (J.rows, J.tensors, J.zero_slices) == (TOWER_B, 32 + nblk, nblk)
