"""Shared by tests/test_e3nn_encoder.py and tests/test_e3nn_fp64_parity.py: the conv calls of the e3nn encoder / prior
written out one by one (what codlad_amd.encoder.Encoder.forward / Prior.forward launch, with host-side CSRs), the float32
oracle's node states before every layer, and the per-receiver, per-channel comparison rule against float64.

The rule (tests/test_fp64_parity.py's, with the channel scale taken per class of receivers):

    err[node, ch] <= c x max(e_ref[ch, class], FLOOR)

err and e_ref are fractions of the channel's largest float64 value over the receivers of the node's class (its degree in
the hand-made graphs: a degree-1 receiver's mean is one message, a degree-200 receiver's an average of 200, and the
first would set the scale of the second); e_ref is the float32 ORACLE's largest error in that channel and class on the
same inputs and never comes from a kernel; c = 4 for the scalar kernel and the small fp32 kernels ("as good as the reference's fp32"), 16 for the
matrix-pipe kernel (operands of 22 of 24 bits: the f16x3 rule); FLOOR = 1e-6 of the channel's scale.
"""
import torch

from oracle import e3nn_lite as e3

FLOOR = 1e-6
C_FP32, C_F16X3 = 4.0, 16.0
RADII = (14.0, 26.0, 26.0)                # atom_max_radius, cg_max_radius, cross_max_distance (utils/model_module.py:22-31)


def block_of(ch):
    return ("0e", "1o", "1e", "0o")[ch // 12]


def device_conv(stack, call, group=None):
    """One `conv` launch of a codlad_amd.encoder stack with accumulate=True into zeros: the device returns the update
    itself.  -> [n_recv, 12 (depth + 2)] on the device."""
    dev = stack.device
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    f = lambda t: None if t is None else t.float().to(dev).contiguous()  # noqa: E731
    ptr, snd = call["csr"]
    assert int(ptr[0]) == 0 and bool((ptr[1:] >= ptr[:-1]).all()) and int(ptr[-1]) <= snd.numel()
    assert snd.numel() > 0 and int(snd.min()) >= 0 and int(snd.max()) < call["xyz_snd"].shape[0] == call["h_snd"].shape[0]
    assert call["xyz_recv"].shape[0] == call["h_recv"].shape[0] == ptr.numel() - 1
    out = torch.zeros(ptr.numel() - 1, 12 * (call["depth"] + 2), dtype=torch.float32, device=dev)
    stack.conv(call["layer"], call["depth"], (d(ptr.int()), d(snd.int())), f(call["xyz_recv"]), f(call["xyz_snd"]),
               f(call["typ_recv"]), f(call["typ_snd"]), call["r_sign"], call["smear_stop"], call["emb"], call["emb_in"],
               f(call["h_recv"]), f(call["h_snd"]), call["recv_first"], out, True, call["group"] if group is None else group)
    return out


def host_csr(recv, snd, n_recv):
    """Edges (recv[e] <- snd[e]) -> (ptr int32 [n_recv + 1], snd int32 [E]), senders ascending inside a receiver: what
    codlad_receiver_csr builds on the device."""
    recv, snd = recv.long(), snd.long()
    order = torch.argsort(recv * (int(snd.max()) + 1 if snd.numel() else 1) + snd)
    ptr = torch.zeros(n_recv + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(recv, minlength=n_recv), 0)
    return ptr.int(), snd[order].int()


def directed_csr(nbr_list, n):
    nb = e3.make_directed(nbr_list)
    return host_csr(nb[:, 0], nb[:, 1], n)


def encoder_graphs(z, xyz, cg_z, cg_xyz, mapping, nbr_list, cg_nbr_list):
    """The four graphs of Encoder.forward as host CSRs, coordinates and types in float32."""
    na, nc = int(z.numel()), int(cg_z.numel())
    return dict(na=na, nc=nc, xa=xyz.float(), xc=cg_xyz.float(), ta=z.float(), tc=cg_z.float(),
                csr_a=directed_csr(nbr_list, na), csr_c=directed_csr(cg_nbr_list, nc),
                csr_c2a=(torch.arange(na + 1, dtype=torch.int32), mapping.int()),
                csr_a2c=host_csr(mapping, torch.arange(na), nc))


def encoder_layer_calls(G, l, ha, hc):
    """The conv calls of layer l of Encoder.forward on node states ha [na, 12 (l + 1)], hc [nc, 12 (l + 1)]: keyword
    arguments of `conv` (and of e3.conv_reference) without out / accumulate, plus `group`."""
    ra, rc, rx = RADII
    calls = [dict(layer=f"atom_conv_layers.{l}", depth=l, csr=G["csr_a"], xyz_recv=G["xa"], xyz_snd=G["xa"], typ_recv=G["ta"],
                  typ_snd=G["ta"], r_sign=1.0, smear_stop=ra, emb="atom_edge_embedding", emb_in=14, h_recv=ha, h_snd=ha,
                  recv_first=True, group=64),
             dict(layer=f"cg_to_atom_conv_layers.{l}", depth=l, csr=G["csr_c2a"], xyz_recv=G["xa"], xyz_snd=G["xc"],
                  typ_recv=None, typ_snd=None, r_sign=-1.0, smear_stop=rx, emb="cross_edge_embedding", emb_in=8, h_recv=ha,
                  h_snd=hc, recv_first=True, group=1)]
    if l != 2:
        calls += [dict(layer=f"cg_conv_layers.{l}", depth=l, csr=G["csr_c"], xyz_recv=G["xc"], xyz_snd=G["xc"], typ_recv=G["tc"],
                       typ_snd=G["tc"], r_sign=1.0, smear_stop=rc, emb="cg_edge_embedding", emb_in=14, h_recv=hc, h_snd=hc,
                       recv_first=True, group=64),
                  dict(layer=f"atom_to_cg_conv_layers.{l}", depth=l, csr=G["csr_a2c"], xyz_recv=G["xc"], xyz_snd=G["xa"],
                       typ_recv=None, typ_snd=None, r_sign=1.0, smear_stop=rx, emb="cross_edge_embedding", emb_in=8, h_recv=hc,
                       h_snd=ha, recv_first=False, group=16)]
    return calls


def reference_of(sd, call, dtype):
    kw = {k: v for k, v in call.items() if k != "group"}
    return e3.conv_reference(sd, dtype=dtype, **kw)


def oracle_layer_states(sd, args):
    """e3.encoder_forward in float32 with the node states every layer starts from kept: -> [(ha, hc)] per layer, and
    the updates {"upd_<layer with _ for .>": tensor} its ten conv layers returned."""
    states, upd, orig = {}, {}, e3.tp_conv_layer

    def spy(sd_, prefix, tp, node_attr, *a, **k):
        out = orig(sd_, prefix, tp, node_attr, *a, **k)
        stack, l = prefix.rsplit(".", 1)
        if stack in ("atom_conv_layers", "cg_to_atom_conv_layers"):
            states[int(l), "a" if stack == "atom_conv_layers" else "c"] = node_attr
        upd["upd_" + prefix.replace(".", "_")] = out
        return out

    e3.tp_conv_layer = spy
    try:
        e3.encoder_forward(sd, *args)
    finally:
        e3.tp_conv_layer = orig
    return [(states[l, "a"], states[l, "c"]) for l in range(3)], upd


def compare(got, ref32, ref64, classes=None):
    """The rule of the module docstring.  got, ref32, ref64 [n, C]; classes int [n] or None (one class) -> dict(ratio =
    the largest err / max(e_ref, FLOOR), node, cls, ch, err, e_ref = of that element, e_lo / e_hi = the range of e_ref over
    channels and classes).  An element whose class has no non-zero float64 value in its channel must be exactly 0."""
    got, r32, r64 = got.detach().cpu().double(), ref32.double(), ref64.double()
    assert got.shape == r32.shape == r64.shape and ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    n, C = r64.shape
    classes = torch.zeros(n, dtype=torch.int64) if classes is None else classes.long()
    scale, e_ref = torch.zeros(n, C, dtype=torch.float64), torch.zeros(n, C, dtype=torch.float64)
    e_all = []
    for k in classes.unique().tolist():
        m = classes == k
        s = r64[m].abs().amax(0)
        e = ((r32[m] - r64[m]).abs() / s.clamp_min(1e-300)).amax(0)
        scale[m], e_ref[m] = s, e
        e_all.append(e[s > 0])
    dead = scale == 0
    assert bool((got[dead] == 0).all()), "a channel that is exactly 0 in float64 for every receiver of a class is not 0"
    ratio = ((got - r64).abs() / scale.clamp_min(1e-300)) / e_ref.clamp_min(FLOOR)
    ratio[dead] = 0.0
    k = int(ratio.argmax())
    node, ch = divmod(k, C)
    e_all = torch.cat(e_all) if e_all else torch.zeros(1, dtype=torch.float64)
    return dict(ratio=float(ratio[node, ch]), node=node, cls=int(classes[node]), ch=ch,
                err=float((got - r64).abs()[node, ch] / scale[node, ch].clamp_min(1e-300)), e_ref=float(e_ref[node, ch]),
                e_lo=float(e_all.min()) if e_all.numel() else 0.0, e_hi=float(e_all.max()) if e_all.numel() else 0.0)


def report(label, res, c, cls_name="degree", blocks=True):
    """Prints the worst element of a comparison and holds it to c."""
    msg = (f"e3nn fp64 parity {label}: err / max(e_ref, FLOOR) {res['ratio']:.2f} (bound {c:g}) at receiver {res['node']} "
           f"({cls_name} {res['cls']}) channel {res['ch']}{' (' + block_of(res['ch']) + ')' if blocks else ''}: err {res['err']:.2e}, e_ref {res['e_ref']:.2e}; "
           f"e_ref over channels and classes {res['e_lo']:.1e} .. {res['e_hi']:.1e}")
    print(msg)
    assert res["ratio"] <= c, msg
    return msg
