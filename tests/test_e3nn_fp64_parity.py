"""GPU: the e3nn encoder / prior kernels against a float64 reference, per launch, receiver and irrep channel.

tests/test_e3nn_encoder.py holds the whole models to the float32 oracle by one max-norm over the final latent.  Here one
`codlad_tp_conv` launch at a time (codlad_amd.encoder's `conv`, accumulate into zeros: the device returns the layer's update
itself) is compared with `oracle.e3nn_lite.conv_reference` in float64 on graphs made for the kernels' edges: the
matrix-pipe kernel (tp_conv_mfma_kernel: 32 edges per step, one receiver per wave, 12 waves per workgroup, a grid capped
at the CU count) and the scalar kernel tp_conv_kernel<DEPTH, G> with G = 64, 16 and 1 lanes per receiver, at every depth.
The rule, its constants and where they come from: tests/e3nn_parity.py.  Then the model's own layers from the device's own
layer inputs (no accumulated error), and the small kernels (codlad_mlp_rows, codlad_bead_mean, codlad_embed_rows) against
float64 directly.

Where a family of launches differs only in how many receivers (rows) it has - 1, 11, 12, 13 ... - all of them are the
leading receivers of ONE pool graph, and the channel scale and e_ref are the pool's: the reference is computed once, and
a launch of a single receiver is not judged relative to that receiver's own, possibly cancelling, value.

Measured ratios of one run: DESIGN.md, "The e3nn conv kernels against float64".
"""
import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth
from oracle import e3nn_lite as e3
from tests import cases
from tests import e3nn_parity as ep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SND = 300
#            name -> (CODLAD_OPT_TP_CONV_VARIANT, group, c)
KERNELS = {"matrix": (0, 64, ep.C_F16X3), "g64": (1, 64, ep.C_FP32), "g16": (1, 16, ep.C_FP32), "g1": (1, 1, ep.C_FP32)}
GRAPH_OF = {"matrix": "wide", "g64": "wide", "g16": "g16", "g1": "g1"}
DEGREES = {"wide": (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 200), "g16": (0, 1, 15, 16, 17, 33), "g1": (0, 1, 2, 7)}
COUNTS = {"matrix": (1, 11, 12, 13), "g64": (1, 2), "g16": (3, 4, 5), "g1": (63, 64, 65)}
KERNEL_DEPTH = [(k, d) for k in KERNELS for d in (0, 1, 2)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _degrees(kind):
    """Receiver degrees of the mixed graphs, at least 8 receivers of every degree, shuffled so that waves and groups hold
    mixed degrees.  g16 (4 receivers per wave): receivers 0 and 1 are of degree 0 and 33, and 50 receivers leave the last
    wave half empty.  g1 (64 receivers per wave): the first wave is all degree 0, the second mixed, the third partial.
    wide: 97 receivers, no multiple of the 12 waves of a workgroup."""
    g = _gen(len(kind))
    rep = torch.tensor(DEGREES[kind]).repeat_interleave({"wide": 8, "g16": 8, "g1": 21}[kind])
    rep = rep[torch.randperm(rep.numel(), generator=g)]
    head = {"wide": [200], "g16": [0, 33], "g1": [0] * 64}[kind]
    return torch.cat([torch.tensor(head), rep])


def _graph(deg, seed, n_snd=N_SND, same_point=0):
    """A valid CSR with the given receiver degrees over random senders (ascending inside a receiver, as
    codlad_receiver_csr leaves them), receivers and senders at random points N(0, 5 A); `same_point`: every
    same_point-th receiver of degree >= 1 sits ON its first sender (r = 0, the CA atom on its bead)."""
    g = _gen(seed)
    n = deg.numel()
    recv = torch.repeat_interleave(torch.arange(n), deg)
    snd = torch.randint(0, n_snd, (recv.numel(),), generator=g)
    csr = ep.host_csr(recv, snd, n)
    xyz_snd, xyz_recv = torch.randn(n_snd, 3, generator=g) * 5.0, torch.randn(n, 3, generator=g) * 5.0
    if same_point:
        for r in torch.nonzero(deg >= 1)[::same_point, 0].tolist():
            xyz_recv[r] = xyz_snd[int(csr[1][int(csr[0][r])])]
    return dict(csr=csr, deg=deg.clone(), xyz_recv=xyz_recv, xyz_snd=xyz_snd,
                typ_recv=torch.randint(1, 21, (n,), generator=g).float(), typ_snd=torch.randint(1, 21, (n_snd,), generator=g).float())


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def graph(kind):
    def make():
        if kind in DEGREES:
            return _graph(_degrees(kind), 100 + len(kind))
        if kind == "pool3":                               # the receiver-count family: 65 receivers of degree 3
            return _graph(torch.full((65,), 3), 7)
        if kind == "persistent":                          # a second pass of the matrix-pipe kernel's persistent loop
            n = 12 * torch.cuda.get_device_properties(0).multi_processor_count + 5
            return _graph(torch.randint(1, 5, (n,), generator=_gen(8)), 9)
        if kind == "bead_to_atom":                        # degree exactly 1, every sixth receiver on its sender
            return _graph(torch.ones(150, dtype=torch.int64), 10, n_snd=20, same_point=6)
        raise KeyError(kind)
    return cached(("graph", kind), make)


def features(kind, depth, variant="plain"):
    """(h_recv [n, 12 (depth + 1)], h_snd [n_snd, 12 (depth + 1)]) for a graph, N(0, 1);
    pow2: each sender's scalar block times its own 2^k, k uniform in -10 .. 10; vec_<s>: the senders' vector blocks times s."""
    def make():
        G = graph(kind)
        g = _gen(1000 + depth)
        n, n_snd, w = G["deg"].numel(), G["xyz_snd"].shape[0], 12 * (depth + 1)
        h_recv, h_snd = torch.randn(n, w, generator=g), torch.randn(n_snd, w, generator=g)
        if variant == "pow2":
            h_snd[:, :12] *= torch.pow(2.0, torch.randint(-10, 11, (n_snd, 1), generator=g).float())
        elif variant.startswith("vec_"):
            h_snd[:, 12:] *= float(variant[4:])
        else:
            assert variant == "plain"
        return h_recv, h_snd
    return cached(("features", kind, depth, variant), make)


SHAPES = {      # the call shapes the models use: name -> (stack, embedding, emb_in, types, recv_first, r_sign, smear_stop)
    "atom": ("atom_conv_layers", "atom_edge_embedding", 14, True, True, 1.0, 14.0),
    "bead": ("cg_conv_layers", "cg_edge_embedding", 14, True, True, 1.0, 26.0),
    "bead_to_atom": ("cg_to_atom_conv_layers", "cross_edge_embedding", 8, False, True, -1.0, 26.0),
    "atom_to_bead": ("atom_to_cg_conv_layers", "cross_edge_embedding", 8, False, False, 1.0, 26.0),
}


def weights(name):
    if name == "trained_c2":
        fix = np.load(cases.npz_path("c2_prior_e3nn"))
        return {k[len("prior_net."):]: torch.from_numpy(fix[k]) for k in fix.files if k.startswith("prior_net.")}
    return synth.encoder_state_dict(41)


def stack_of(name="synthetic"):
    from codlad_amd.encoder import Encoder, Prior
    return cached(("stack", name), lambda: (Prior if name == "trained_c2" else Encoder)(weights(name), DEV))


def call_of(kind, depth, shape="atom", variant="plain", n_recv=None):
    """The keyword arguments of one conv launch (tests/e3nn_parity.py device_conv / reference_of), optionally of the first
    n_recv receivers of the graph alone."""
    G = graph(kind)
    stack, emb, emb_in, types, recv_first, r_sign, stop = SHAPES[shape]
    h_recv, h_snd = features(kind, depth, variant)
    ptr, snd = G["csr"]
    n = G["deg"].numel() if n_recv is None else n_recv
    return dict(layer=f"{stack}.{depth}", depth=depth, csr=(ptr[:n + 1], snd), xyz_recv=G["xyz_recv"][:n], xyz_snd=G["xyz_snd"],
                typ_recv=G["typ_recv"][:n] if types else None, typ_snd=G["typ_snd"] if types else None, r_sign=r_sign,
                smear_stop=stop, emb=emb, emb_in=emb_in, h_recv=h_recv[:n], h_snd=h_snd, recv_first=recv_first, group=64)


def references(key, call, wname="synthetic"):
    """(float32, float64) conv_reference of a call, computed once per key and left unchanged."""
    def make():
        sd = weights(wname)
        r32, r64 = ep.reference_of(sd, call, torch.float32), ep.reference_of(sd, call, torch.float64)
        assert r32.dtype == torch.float32 and r64.dtype == torch.float64
        return r32, r64
    return cached(("ref", wname) + key, make)


def launch(kernel, call, wname="synthetic", pack=True):
    variant, group, _c = KERNELS[kernel]
    stack = stack_of(wname)
    _lib.set_option(_lib.OPT_TP_CONV_VARIANT, variant)
    stack.pack_weights = pack
    try:
        out = ep.device_conv(stack, call, group)
        torch.cuda.synchronize()
    finally:
        stack.pack_weights = True
        _lib.set_option(_lib.OPT_TP_CONV_VARIANT, 0)
    return out.cpu()


def hold(label, kernel, got, refs, deg):
    assert bool(torch.isfinite(got).all()), label
    assert bool((got[deg == 0] == 0).all()), f"{label}: a receiver without an edge must return exactly 0"
    return ep.report(f"{label} {kernel}", ep.compare(got, refs[0], refs[1], deg), KERNELS[kernel][2])


def mixed_output(kernel, depth):
    call = call_of(GRAPH_OF[kernel], depth)
    return call, cached(("out", kernel, depth), lambda: launch(kernel, call))


# --------------------------------------------------------------------------------------------------- one launch: degrees
@pytest.mark.parametrize("kernel,depth", KERNEL_DEPTH)
def test_one_launch_against_float64_on_mixed_degrees(kernel, depth):
    """Receivers of degree 0, 1, 2 and around every multiple of the kernel's step (32 edges for the matrix pipe, G lanes
    for the scalar kernel) in one launch, each degree class judged on its own scale."""
    kind = GRAPH_OF[kernel]
    G = graph(kind)
    assert all(int((G["deg"] == d).sum()) >= 8 for d in DEGREES[kind])
    if kind == "g16":
        assert G["deg"][:2].tolist() == [0, 33]
    if kind == "g1":
        assert bool((G["deg"][:64] == 0).all())
    call, got = mixed_output(kernel, depth)
    hold(f"mixed degrees depth {depth}", kernel, got, references((kind, depth, "atom", "plain"), call), G["deg"])


@pytest.mark.parametrize("kernel,depth", KERNEL_DEPTH)
def test_rows_are_reproducible_and_do_not_depend_on_the_launch(kernel, depth):
    """Two runs give equal bits, and a receiver's row is the same when the receiver is launched alone (n_recv = 1, its
    own CSR): the kernels sum a receiver's edges in a fixed order whatever shares the launch."""
    kind = GRAPH_OF[kernel]
    G = graph(kind)
    call, got = mixed_output(kernel, depth)
    assert torch.equal(launch(kernel, call), got)
    ptr, snd = G["csr"]
    top = int(G["deg"].max())
    picks = [int(torch.nonzero(G["deg"] == top)[-1]), int(torch.nonzero(G["deg"] == DEGREES[kind][-2])[0]), G["deg"].numel() - 1]
    for r in picks:
        a, b = int(ptr[r]), int(ptr[r + 1])
        alone = dict(call, csr=(torch.tensor([0, b - a], dtype=torch.int32), snd[a:b] if b > a else snd[:1]),
                     xyz_recv=call["xyz_recv"][r:r + 1], typ_recv=call["typ_recv"][r:r + 1], h_recv=call["h_recv"][r:r + 1])
        assert torch.equal(launch(kernel, alone)[0], got[r]), f"{kernel} depth {depth}: receiver {r} (degree {b - a}) alone"


# --------------------------------------------------------------------------------------------------- one launch: counts
@pytest.mark.parametrize("kernel,depth", KERNEL_DEPTH)
def test_one_launch_against_float64_receiver_counts(kernel, depth):
    """Receiver counts around the kernels' receivers per wave / workgroup (12 for the matrix pipe, 4 for G = 16, 64 for
    G = 1; G = 64 has one receiver per workgroup): the leading receivers of one degree-3 pool graph."""
    G = graph("pool3")
    refs = references(("pool3", depth, "atom", "plain"), call_of("pool3", depth))
    for n in COUNTS[kernel]:
        got = launch(kernel, call_of("pool3", depth, n_recv=n))
        assert got.shape[0] == n
        # the pool's scale and e_ref: the rows that were not launched are filled with the reference's own
        res = ep.compare(torch.cat([got.double(), refs[1][n:]]), refs[0], refs[1], G["deg"])
        ep.report(f"{n} receivers of degree 3, depth {depth} {kernel}", res, KERNELS[kernel][2])
        assert res["node"] < n or res["ratio"] == 0.0


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_matrix_pipe_second_persistent_pass(depth):
    """12 x CU count + 5 receivers of degree 1 to 4: every wave of the capped grid takes a second receiver, and the
    per-wave output row in LDS is reused."""
    G = graph("persistent")
    call = call_of("persistent", depth)
    hold(f"persistent loop, {G['deg'].numel()} receivers, depth {depth}", "matrix", launch("matrix", call),
         references(("persistent", depth, "atom", "plain"), call), G["deg"])


# --------------------------------------------------------------------------------------------------- the models' call shapes
@pytest.mark.parametrize("shape,kind,scalar", [("atom", "wide", "g64"), ("bead", "wide", "g64"), ("bead_to_atom", "bead_to_atom", "g1"),
                                               ("atom_to_bead", "g16", "g16")])
def test_call_shapes_of_the_models_depth_1(shape, kind, scalar):
    """With / without node types in a 14- / 8-wide edge embedding, both attribute orders, both signs of r, both smearing
    ranges - on the matrix pipe and on the scalar group the model uses; weights packed once or by every workgroup: the same
    bits.  bead_to_atom: degree exactly 1, every sixth edge of length 0."""
    G = graph(kind)
    call = call_of(kind, 1, shape)
    if shape == "bead_to_atom":
        ptr, snd = G["csr"]
        zero = ((G["xyz_recv"] - G["xyz_snd"][snd.long()]).abs().amax(-1) == 0).sum()
        assert bool((G["deg"] == 1).all()) and int(zero) == 25
    refs = references((kind, 1, shape, "plain"), call)
    for kernel in ("matrix", scalar):
        got = launch(kernel, call)
        hold(f"{shape} depth 1", kernel, got, refs, G["deg"])
        assert torch.equal(launch(kernel, call, pack=False), got), f"{shape} {kernel}: pack_weights False"


# --------------------------------------------------------------------------------------------------- magnitudes
@pytest.mark.parametrize("kernel", ["matrix", "g64"])
@pytest.mark.parametrize("variant", ["pow2", "vec_0.001", "vec_1000.0"])
def test_magnitudes_depth_2(kernel, variant):
    """The matrix-pipe kernel scales each edge's 37 fc inputs and 36 hidden units by the edge's own power of two (floor
    1.0).  pow2: every sender's scalars times its own 2^k, k = -10 .. 10, so that edges of very different input scale
    share a 32-edge step; vec_<s>: the vector blocks of all senders times s.

    pow2-g64 is the regression test of a finding: with fc's two layers accumulated in fp32 the scalar kernel read 6.04
    against c = 4 at receiver 24 (degree 1), channel 16 (1o), and 4.81 at channel 17 (the matrix pipe 9.53 of 16 at the
    same element).  That receiver's only sender carries 2^10 and its second 1o output (236, 59.5, -119) is what is left
    of terms thirty times larger, so every rounding of fc's 36 x 16 products shows there.  tp_conv_kernel now accumulates
    fc.0, fc.3 and the path sums in float64 (encoder_kernels.hip) and reads 0.59 ("The e3nn conv kernels
    against float64")."""
    G = graph("wide")
    call = call_of("wide", 2, variant=variant)
    hold(f"{variant} depth 2", kernel, launch(kernel, call), references(("wide", 2, "atom", variant), call), G["deg"])


@pytest.mark.parametrize("kernel", ["matrix", "g64"])
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_trained_c2_prior_weights(kernel, depth):
    """cg_conv_layers.{0, 1, 2} of the shipped C2 prior (tests/golden/c2_prior_e3nn.npz) on the mixed-degree graph."""
    G = graph("wide")
    call = call_of("wide", depth, "bead")
    hold(f"trained C2 prior depth {depth}", kernel, launch(kernel, call, "trained_c2"),
         references(("wide", depth, "bead", "plain"), call, "trained_c2"), G["deg"])


# --------------------------------------------------------------------------------------------------- the models' own layers
def _recording(cls, sd):
    class Recording(cls):
        """Keeps every conv call's arguments, the state it found in `out` and the state it left there."""
        calls = None

        def conv(self, layer, depth, csr, xyz_recv, xyz_snd, typ_recv, typ_snd, r_sign, smear_stop, emb, emb_in, h_recv, h_snd,
                 recv_first, out, accumulate, group):
            c = lambda t: None if t is None else t.detach().cpu().clone()  # noqa: E731
            base = c(out) if accumulate else torch.nn.functional.pad(c(h_recv), (0, out.shape[1] - h_recv.shape[1]))
            super().conv(layer, depth, csr, xyz_recv, xyz_snd, typ_recv, typ_snd, r_sign, smear_stop, emb, emb_in, h_recv, h_snd,
                         recv_first, out, accumulate, group)
            self.calls.append((dict(layer=layer, depth=depth, csr=(c(csr[0]), c(csr[1])), xyz_recv=c(xyz_recv), xyz_snd=c(xyz_snd),
                                    typ_recv=c(typ_recv), typ_snd=c(typ_snd), r_sign=r_sign, smear_stop=smear_stop, emb=emb,
                                    emb_in=emb_in, h_recv=c(h_recv), h_snd=c(h_snd), recv_first=recv_first, group=group),
                               base, c(out)))
    net = Recording(sd, DEV)
    net.calls = []
    return net


@pytest.mark.parametrize("model,variant", [("encoder_L46x2", 0), ("encoder_L46x2", 2), ("prior_seeded_L129", 0)])
def test_model_layers_from_their_own_inputs(model, variant):
    """Encoder.forward / Prior.forward with every conv call's input and output state read back: each of the ten / three
    launches is given to the float64 and the float32 conv_reference with the DEVICE's own input state (cast up), so no
    error accumulates over the layers, and the state it leaves (its base - the padded input or what the intra-level conv left
    - plus the update) is compared by the rule: the floor is on the state's scale, channels are scaled over all receivers.
    CODLAD_OPT_TP_CONV_VARIANT 0 (as shipped): every graph on the matrix pipe, c = 16; 2: the cross graphs (group 1 and 16)
    on the scalar kernel, c = 4 there (the prior has no cross graph)."""
    _lib.set_option(_lib.OPT_TP_CONV_VARIANT, variant)
    try:
        if model.startswith("encoder"):
            from codlad_amd.encoder import Encoder
            L, frames, wseed = cases.E3NN_ENCODER_CASES[model[len("encoder_"):]]
            sd = synth.encoder_state_dict(wseed)
            prot = synth.make_protein(L, 50 + L, n_frames=frames)
            batch, atoms = synth.make_batch(prot), synth.make_atoms(prot, seed=L)
            net = _recording(Encoder, sd)
            net.forward(atoms["nxyz"][:, 0], atoms["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                        atoms["CG_mapping"], atoms["nbr_list"], batch["CG_nbr_list"])
        else:
            from codlad_amd.encoder import Prior
            L, frames, wseed, _w = cases.E3NN_PRIOR_CASES[model[len("prior_"):]]
            sd = synth.prior_state_dict(wseed)
            batch = synth.make_batch(synth.make_protein(L, 40 + L, n_frames=frames))
            net = _recording(Prior, sd)
            net.forward(batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"])
        torch.cuda.synchronize()
    finally:
        _lib.set_option(_lib.OPT_TP_CONV_VARIANT, 0)
    assert len(net.calls) == (10 if model.startswith("encoder") else 3)
    for call, base, state in net.calls:
        refs = ep.reference_of(sd, call, torch.float32), ep.reference_of(sd, call, torch.float64)       # from this run's own states
        matrix = variant == 0 or call["group"] == 64
        res = ep.compare(state, base + refs[0], base.double() + refs[1])
        ep.report(f"{model} {call['layer']} ({'matrix' if matrix else 'g%d' % call['group']})", res,
                  ep.C_F16X3 if matrix else ep.C_FP32, cls_name="class")


# --------------------------------------------------------------------------------------------------- the small kernels
ROWS = (1, 63, 64, 65, 200)


def _mlp_stack():
    """A stack whose blob holds heads of the shapes the models use, with first layers large enough to saturate tanh:
    pre-activations of N(0, 7), up to about +-20."""
    def make():
        from codlad_amd.encoder import Encoder
        g = _gen(77)
        sd = dict(synth.encoder_state_dict(41))
        for name, n_in in (("m84", 84), ("m48", 48)):
            sd[f"{name}.0.weight"] = torch.randn(36, n_in, generator=g) * (7.0 / n_in ** 0.5)
            sd[f"{name}.0.bias"] = torch.randn(36, generator=g)
            sd[f"{name}.2.weight"] = torch.randn(36, 36, generator=g) / 6.0
            sd[f"{name}.2.bias"] = torch.randn(36, generator=g) * 0.1
        sd["lin.weight"], sd["lin.bias"] = torch.randn(3, 36, generator=g) / 6.0, torch.randn(3, generator=g)
        return Encoder(sd, DEV), sd
    return cached("mlp", make)


def _mlp_reference(sd, x, first, second, mode):
    """torch in the dtype of x."""
    w = lambda k: sd[k].to(x.dtype)  # noqa: E731
    if first is not None:
        x = torch.tanh(torch.nn.functional.linear(x, w(first + ".weight"), w(first + ".bias")))
    y = torch.nn.functional.linear(x, w(second + ".weight"), w(second + ".bias"))
    return 1e-9 + torch.exp(y / 2) if mode == 1 else y


@pytest.mark.parametrize("first,second,n_in,mode", [("m84.0", "m84.2", 84, 0), ("m48.0", "m48.2", 48, 0), ("m48.0", "m48.2", 48, 1),
                                                     (None, "lin", 36, 0)])
def test_mlp_rows_against_float64(first, second, n_in, mode):
    """codlad_mlp_rows (64 rows per workgroup): the dense head (84 -> 36 -> 36, tanh), the prior's heads (48 -> 36 -> 36;
    mode 1 = the sigma head, 1e-9 + exp(y / 2)) and a single Linear, at row counts around 64, the rows being the leading
    rows of one pool of 200."""
    stack, sd = _mlp_stack()
    x = torch.randn(ROWS[-1], n_in, generator=_gen(n_in + mode))
    if first is not None:
        pre = torch.nn.functional.linear(x.double(), sd[first + ".weight"].double(), sd[first + ".bias"].double()).abs()
        assert 15.0 < float(pre.max()) and float((pre > 9.0).double().mean()) > 0.1          # tanh saturates in fp32 beyond ~9
    r32, r64 = _mlp_reference(sd, x, first, second, mode), _mlp_reference(sd, x.double(), first, second, mode)
    for n in ROWS:
        got = stack.mlp(x[:n].to(DEV), first, second, "tanh", mode=mode).cpu()
        assert got.shape == (n, r64.shape[1])
        res = ep.compare(torch.cat([got.double(), r64[n:]]), r32, r64)            # the pool's scale and e_ref
        ep.report(f"mlp_rows {n_in} -> {second} mode {mode}, {n} rows", res, ep.C_FP32, cls_name="class", blocks=False)


def test_bead_mean_against_float64():
    """codlad_bead_mean: beads of 1, 2, 24 and 70 atoms (their atoms scattered over the atom list) against the float64
    mean of cat([ha, hc[mapping]]), each bead size judged on its own scale."""
    L = _lib
    g = _gen(5)
    sizes = torch.tensor([1, 2, 24, 70]).repeat(5)[torch.randperm(20, generator=g)]
    mapping = torch.repeat_interleave(torch.arange(20), sizes)
    mapping = mapping[torch.randperm(mapping.numel(), generator=g)]
    na = mapping.numel()
    ha, hc = torch.randn(na, 48, generator=g), torch.randn(20, 36, generator=g)
    ptr, atoms = ep.host_csr(mapping, torch.arange(na), 20)
    node = torch.empty(20, 84, device=DEV)
    L.check(L.lib().codlad_bead_mean(L.ptr(ha.to(DEV)), L.ptr(hc.to(DEV)), L.ptr(ptr.to(DEV)), L.ptr(atoms.to(DEV)), 20,
                                     L.ptr(node), L.stream_ptr(torch.device(DEV))), "codlad_bead_mean")
    torch.cuda.synchronize()
    r32 = e3.scatter_mean(torch.cat([ha, hc[mapping]], -1), mapping, 20)
    r64 = e3.scatter_mean(torch.cat([ha.double(), hc.double()[mapping]], -1), mapping, 20)
    ep.report("bead_mean", ep.compare(node, r32, r64, sizes), ep.C_FP32, cls_name="bead size", blocks=False)
    assert torch.equal(node[:, 48:].cpu(), hc)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_embed_rows_is_exact(n):
    stack, sd = _mlp_stack()
    idx = torch.randint(0, 30, (n,), generator=_gen(n))
    got = stack.embed("atom_node_embedding.weight", idx.to(DEV))
    assert torch.equal(got.cpu(), sd["atom_node_embedding.weight"][idx])
