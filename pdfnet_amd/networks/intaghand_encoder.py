"""MI355X-native counterpart of the reference's lib/models/networks/intaghand_encoder.py:
ResNet-50 RGB trunk + pyramid fusion + PointNet++ set abstraction on the depth cloud + SFT fusion.

Same module tree / state_dict keys as the reference `ResNetSimple` (intaghand_encoder.py:567-819) and
`resnet_mid` (:822-881); every op is a HIP kernel through pdfnet_amd.functional.  Internally all maps are
NHWC (channels_last) and point features are row-major [cloud, point, channel].
"""
import torch
import torch.nn as nn

import os

from .. import functional as F
from .layers import (BatchNorm, Conv2d, ConvTranspose2d, Linear, PointConv, Slot, kaiming_normal_, small_normal_)


def _pad16(c):
    return (c + 15) // 16 * 16


LAZY_TRUNK_BN = os.environ.get("PDFNET_LAZY_TRUNK_BN", "1") != "0"


class Bottleneck(nn.Module):
    """ResNet v1.5 bottleneck, stride on conv2 (reference twin lib/models/networks/resnet.py:76-122)."""

    def __init__(self, cin, width, stride, down):
        super().__init__()
        self.conv1 = Conv2d(cin, width, 1, bias=False)
        self.bn1 = BatchNorm(width)
        self.conv2 = Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = BatchNorm(width)
        self.conv3 = Conv2d(width, width * 4, 1, bias=False)
        self.bn3 = BatchNorm(width * 4)
        self.downsample = None
        if down:
            self.downsample = nn.Sequential(Conv2d(cin, width * 4, 1, stride, 0, bias=False), BatchNorm(width * 4))

    def forward(self, x):
        # every convolution feeds a BatchNorm: statistics in the GEMM epilogue -- asked for by the CONSUMING BatchNorm's own mode
        # (a frozen `bn.eval()` inside a train-mode block must read a materialised tensor)
        if x.requires_grad:
            # conv1 hands the input back as the shortcut's source so both gradients of x meet in conv1's backward, which
            # accumulates onto the shortcut's gradient (identity, or the projection's backward-data) in the GEMM epilogue
            # -- no separate add pass over the block input's gradient
            y, sc = F.conv2d_with_skip(x, self.conv1.weight, None, 1, 0, stats=self.bn1.training)
        else:
            y, sc = self.conv1(x, stats=self.bn1.training), x
        y = self.bn1(y, relu=True)
        y = self.conv2(y, stats=self.bn2.training)
        if LAZY_TRUNK_BN and self.bn2.training and y.requires_grad and not F._GEMM_BF16:
            # relu(bn2(.)) has ONE consumer and it is a 1x1 convolution -- a linear layer over the NHWC rows: the normalised tensor is
            # never written; conv3 applies scale / shift / ReLU while it stages its rows, forward and weight gradient (F.batch_norm lazy,
            # the set-abstraction MLPs' arrangement; VERDICT r4 item 3, the part of it that needs no new kernel)
            n_, c_, h_, w_ = y.shape
            z = self.bn2(F.carry_stats(y, y.permute(0, 2, 3, 1).reshape(-1, c_)), relu=True, lazy=True)
            y3 = F.linear(z, F.as_matrix(self.conv3.weight), None, stats=self.bn3.training)
            y = F.carry_stats(y3, y3.view(n_, h_, w_, -1).permute(0, 3, 1, 2))
        else:
            y = self.conv3(self.bn2(y, relu=True), stats=self.bn3.training)
        if self.downsample is not None:
            sc = self.downsample[1](self.downsample[0](sc, stats=self.downsample[1].training))
        return self.bn3(y, relu=True, res=sc)          # relu(bn3(y) + shortcut) in one pass


class ResNet50(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = BatchNorm(64)
        cin = 64
        for li, (width, n, stride) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)], 1):
            blocks = []
            for b in range(n):
                blocks.append(Bottleneck(cin, width, stride if b == 0 else 1, b == 0))
                cin = width * 4
            setattr(self, "layer%d" % li, nn.Sequential(*blocks))
        self.fc = Linear(2048, 1000)               # key parity only (never on the path)
        for m in self.modules():                   # torchvision init
            if isinstance(m, Conv2d):
                nn.init.kaiming_normal_(m.weight.data, mode='fan_out', nonlinearity='relu')


class L2Norm(nn.Module):
    def __init__(self, c, scale):
        super().__init__()
        self.weight = nn.Parameter(torch.full((c,), float(scale)))

    def forward(self, x):
        return F.l2norm(x, self.weight, 1e-10)


class SFTLayer(nn.Module):
    """intaghand_encoder.py:205-219 on rows: fea [.., P, Cf], cond [.., P, Cc] -> [.., P, Cf]."""

    def __init__(self, c_fea, c_cond):
        super().__init__()
        self.SFT_scale_conv0 = PointConv(c_cond, c_cond)
        self.SFT_scale_conv1 = PointConv(c_cond, c_fea)
        self.SFT_shift_conv0 = PointConv(c_cond, c_cond)
        self.SFT_shift_conv1 = PointConv(c_cond, c_fea)

    def forward(self, fea, cond):
        if fea.shape[-1] == 3 and cond.shape[-1] == 3:           # sft0: one kernel per direction for the whole layer
            convs = (self.SFT_scale_conv0, self.SFT_scale_conv1, self.SFT_shift_conv0, self.SFT_shift_conv1)
            return F.sft3(fea, cond, [t for c in convs for t in (c.weight, c.bias)])
        # fea may arrive zero-padded to a multiple of 16 channels: scale / shift are produced at that width (zero in the padding,
        # so the padding stays zero) and every GEMM of the layer keeps 16-byte aligned rows
        npad = fea.shape[-1]
        scale = self.SFT_scale_conv1(self.SFT_scale_conv0(cond, F.ACT_LRELU), npad=npad)
        shift = self.SFT_shift_conv1(self.SFT_shift_conv0(cond, F.ACT_LRELU), npad=npad)
        return F.sft_modulate(fea, scale, shift)


def _sa_mlp(cin, dims):
    mods = []
    for d in dims:
        mods += [PointConv(cin, d), BatchNorm(d), Slot()]
        cin = d
    return mods + [Slot()]          # index 9 = the reference's MaxPool2d slot




# the inner BatchNorm + ReLU of the set-abstraction MLPs applied by the consuming linear layer (F.batch_norm lazy=True)
LAZY_SA_BN = os.environ.get("PDFNET_LAZY_SA_BN", "0") != "0"     # (opt-in: measured neutral in time)


class PointNet_Plus(nn.Module):
    """intaghand_encoder.py:32-159.  One call per hand (BN batch statistics are per hand, :805-806)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.sft0, self.sft1, self.sft2 = SFTLayer(3, 3), SFTLayer(131, 64), SFTLayer(259, 256)
        self.netR_1 = nn.Sequential(*_sa_mlp(opt.INPUT_FEATURE_NUM, [64, 64, 128]))
        self.netR_2 = nn.Sequential(*_sa_mlp(131, [128, 128, 256]))
        self.netR_3 = nn.Sequential(*_sa_mlp(259, [512, 512, 1024]))
        self.netR_FC = nn.Sequential(Linear(1024, 1024), BatchNorm(1024), Slot(), Linear(1024, 512), BatchNorm(512), Slot(),
                                     Linear(512, opt.PCA_SZ))          # constructed, unused (:155)

    @staticmethod
    def _mlp_max(seq, y1, K):
        """Rest of a set-abstraction MLP after its first 1x1 convolution (:48-65,67-103): BN -> ReLU, 2 x (conv -> BN -> ReLU),
        MaxPool over the K neighbours.  y1: rows [cloud*centroid*neighbour, channel].  The last BatchNorm, its ReLU and the
        pooling are one pass over the last convolution's output (F.bn_relu_max_over_k)."""
        # (lazy: the two inner BatchNorm + ReLU are applied by the linear layer that consumes them -- no pass over the rows, no
        # normalised tensor; F.batch_norm)
        x = seq[1](F.carry_stats(y1, y1.reshape(-1, y1.shape[-1])), relu=True, lazy=LAZY_SA_BN)
        x = seq[4](seq[3](x, stats=seq[4].training), relu=True, lazy=LAZY_SA_BN)
        return seq[7].relu_max_over_k(seq[6](x, stats=seq[7].training), K)

    @staticmethod
    def _sa_fused_on(seq, rows):
        """F.SA_FUSED (PDFNET_SA_FUSED / F.set_sa_fused): levels 1 and 2 run as ONE fused MLP with recomputation (F.sa_mlp_fused) --
        fp32 mode only: under the bf16 GEMM precision the per-layer path below is kept.  PDFNET_LAZY_SA_BN does not apply to it.
        The fused backward exists for batch statistics only: a level whose BatchNorms are frozen (eval mode) and whose input rows
        want a gradient takes the per-layer path, which has the frozen-statistics backward."""
        bns = (seq[1], seq[4], seq[7])
        if not (F.SA_FUSED and not F._GEMM_BF16 and bns[0].training == bns[1].training == bns[2].training):
            return False
        return bns[0].training or not (torch.is_grad_enabled() and rows.requires_grad)

    @staticmethod
    def _sa_fused(seq, rows, S, K, r2):
        """The whole MLP of a level (:48-65 / :67-85) on the fused kernels: first 1x1 convolution per POINT (as in _group_conv), then
        F.sa_mlp_fused -- no [rows, C] activation is kept between forward and backward.  -> [B*S, C3]."""
        idx = F.knn_ball_indices(rows, S, K, r2)
        conv = seq[0]
        w = conv.matrix(rows.shape[-1])
        u = F.linear(rows, w, conv.bias, fp32=True)
        ctr = torch.nn.functional.pad(rows[:, :S, :3], (0, rows.shape[-1] - 3))
        v = F.linear(ctr, w, fp32=True)
        bns = (seq[1], seq[4], seq[7])
        for bn in bns:
            bn.track_call()
        return F.sa_mlp_fused(u, v, idx, seq[3].weight.flatten(1), seq[3].bias, seq[6].weight.flatten(1), seq[6].bias,
                              *[bn.weight for bn in bns], *[bn.bias for bn in bns],
                              *[t for bn in bns for t in (bn.running_mean, bn.running_var)], bns[0].training, bns[0].momentum, bns[0].eps)

    @staticmethod
    def _group_conv(conv, rows, S, K, r2):
        """group_points / group_points_2 (lib/utils/utils.py:134-188) followed by the MLP's first 1x1 convolution, without the
        grouped tensor: the convolution is linear, so it is applied once per POINT and its rows are gathered --
        conv(p_idx - centre_xyz) = conv(p)[idx] - W[:, :3] centre_xyz (F.gather_sub).  rows [B,N,Cpad]: xyz first, zero-padded to
        a multiple of 16 channels.  -> [B,S,K,Cout] (pre-BatchNorm)."""
        idx = F.knn_ball_indices(rows, S, K, r2)                                           # kNN + ball rule on (modulated) xyz
        w = conv.matrix(rows.shape[-1])
        # fp32 also in bf16 mode: the layer sees ABSOLUTE coordinates (0.45 +- 0.1 m) whose differences (centimetres) carry the
        # signal; rounding them to bf16 (2 mm steps) before the subtraction would destroy it.  N rows: the cost is nothing.
        u = F.linear(rows, w, conv.bias, fp32=True)                                        # [B,N,Cout]
        ctr = torch.nn.functional.pad(rows[:, :S, :3], (0, rows.shape[-1] - 3))            # centres = the first S points
        return F.gather_sub(u, F.linear(ctr, w, fp32=True), idx)

    def forward(self, cloud, emb, choose):
        return self.stage_b(*self.stage_a(cloud, emb[0], emb[1], choose), emb[2], choose)

    def stage_a(self, cloud, emb0, emb1, choose, chain=False):
        """Set-abstraction levels 1 and 2 (:120-145).  They read only the two shallow embeddings (e_conv1 and the stem), so
        the encoder starts them on a side stream next to the ResNet trunk: HBM-bound point kernels under MFMA-bound convs."""
        o = self.opt
        R, S1, S2, K = o.default_resolution, o.sample_num_level1, o.sample_num_level2, o.knn_K
        B = cloud.shape[0]
        # chain=True: also returns emb0 / emb1 for the NEXT consumer of these maps (the other hand): the scatter-type backward
        # passes of all consumers then fill one gradient tensor per map (F.gather_rows)
        e0 = F.gather_rows(emb0, choose, chain=chain)
        if chain:
            e0, emb0 = e0
        pts = self.sft0(cloud, e0)                                                         # [B,1024,3]   (:120-122)
        rows1 = F.pad2d(pts.reshape(-1, 3), pts.shape[0] * pts.shape[1], _pad16(3)).view(pts.shape[0], pts.shape[1], _pad16(3))
        if self._sa_fused_on(self.netR_1, rows1):
            x = self._sa_fused(self.netR_1, rows1, S1, K, o.ball_radius)                    # [B*S1,128]
        else:
            y1 = self._group_conv(self.netR_1[0], rows1, S1, K, o.ball_radius)             # (:123,:49)
            x = self._mlp_max(self.netR_1, y1, K)                                           # [B*S1,128]   (:132)
        e1 = F.gather_rows(emb1, choose[:, :S1], R, 1, chain=chain)                        # [B,S1,64]    (:125-127)
        if chain:
            e1, emb1 = e1
        x = torch.cat((pts[:, :S1], x.view(B, S1, 128), x.new_zeros(B, S1, _pad16(131) - 131)), 2)   # [B,S1,131 | 0]   (:134)
        x = self.sft1(x, e1)                                                               #              (:137)
        if self._sa_fused_on(self.netR_2, x):
            y = self._sa_fused(self.netR_2, x, S2, K, o.ball_radius2)                        # [B*S2,256]
        else:
            y1 = self._group_conv(self.netR_2[0], x, S2, K, o.ball_radius2)                # (:139,:68)
            y = self._mlp_max(self.netR_2, y1, K)                                           # [B*S2,256]
        return (x, y, emb0, emb1) if chain else (x, y)

    def stage_b(self, x, y, emb2, choose, chain=False):
        """Level 3 (:146-152): needs the fused pyramid feature map x0."""
        o = self.opt
        R, S2 = o.default_resolution, o.sample_num_level2
        B = x.shape[0]
        e2 = F.gather_rows(emb2, choose[:, :S2], R, 2, chain=chain)                        # [B,S2,256]   (:126,128)
        if chain:
            e2, emb2 = e2
        y = torch.cat((x[:, :S2, :3], y.view(B, S2, 256), y.new_zeros(B, S2, _pad16(259) - 259)), 2)   # [B,S2,259 | 0]
        y = self.sft2(y, e2)                                                               #              (:147)
        y = self._mlp_max(self.netR_3, self.netR_3[0](y, stats=self.netR_3[1].training), S2)           # [B,1024]     (:152)
        return (y.view(B, 1, 1024), emb2) if chain else y.view(B, 1, 1024)


class ResNetSimple_decoder(nn.Module):
    """intaghand_encoder.py:270-316: 1x1 then 3 x [bilinear x2 -> conv3x3 -> ReLU -> BN] (conv->ReLU->BN order)."""

    def __init__(self, out_dim, up_scale):
        super().__init__()
        self.models = nn.ModuleList([nn.Sequential(Conv2d(2048, 128, 1, bias=False), Slot(), BatchNorm(128))])
        for _ in range(3):
            self.models.append(nn.Sequential(Slot(), Conv2d(128, 128, 3, 1, 1, bias=False), Slot(), BatchNorm(128)))
        self.up_scale = up_scale
        if up_scale:
            self.final_layer = nn.Sequential(Slot(), Conv2d(128, out_dim, 1), Slot())
        else:
            self.final_layer = nn.Sequential(Conv2d(128, out_dim, 1))
        kaiming_normal_(self)

    def forward(self, x):
        fmaps = []
        x = self.models[0][2](self.models[0][0](x, F.ACT_RELU, stats=self.models[0][2].training))
        fmaps.append(x)
        for m in list(self.models)[1:]:
            x = m[3](m[1](F.upsample2x(x), F.ACT_RELU, stats=m[3].training))
            fmaps.append(x)
        if self.up_scale:
            x = F.upsample2x(self.final_layer[1](F.upsample2x(x)))
        else:
            x = self.final_layer[0](x)
        return x, fmaps


def _fc_head(dout):
    return nn.Sequential(Linear(1024, 512), BatchNorm(512), Slot(), Linear(512, 256), BatchNorm(256), Slot(), Linear(256, dout))


def nms_top1_centers(hm):
    """Centre pick of the test path (intaghand_encoder.py:349-367,750-758): 5x5 max-pool NMS on the raw logits,
    top-1 per channel -- one HIP kernel (pdf_nms_top1)."""
    return F.nms_top1(hm)[0]


class ResNetSimple(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.on_trunk_output_grad = None        # set by the trainer: overlaps the gradient all-reduce with the trunk's backward
        self.resnet = ResNet50()
        self.p2 = Conv2d(256, 256, 3, 1, 1)
        self.p3 = ConvTranspose2d(512, 256, 4, 2, 1)
        self.p4 = ConvTranspose2d(1024, 256, 4, 4, 0)
        self.p5 = ConvTranspose2d(2048, 256, 8, 8, 0)
        self.p2_l2, self.p3_l2, self.p4_l2, self.p5_l2 = (L2Norm(256, 10) for _ in range(4))
        self.feat = Conv2d(1024, 256, 3, 1, 1, bias=False)
        self.feat_bn = BatchNorm(256, momentum=0.01)
        self.e_conv1 = Conv2d(3, 3, 3, 1, 1, bias=False)
        self.pointnet_plus = PointNet_Plus(opt)
        self.hms_decoder = ResNetSimple_decoder(42, False)
        self.center_feat_up0 = Conv2d(256, 512, 3, 1, 1, bias=False)
        self.center_feat_up1 = Conv2d(512, 1024, 3, 1, 1, bias=False)
        self.mano_head, self.joint_head_l, self.joint_head_r = _fc_head(122), _fc_head(66), _fc_head(66)   # unused (:811)
        for m in (self.mano_head, self.joint_head_l, self.joint_head_r):
            small_normal_(m)
        self.sft = SFTLayer(1024, 1024)
        for head in sorted(opt.heads):
            fc = nn.Sequential(Conv2d(256, 256, 3, 1, 1), Slot(), Conv2d(256, opt.heads[head], 1))
            if 'hm' in head:
                fc[2].bias.data.fill_(-4.59)                   # :690
            else:
                small_normal_(fc)
            setattr(self, head, fc)
        self.dp_decoder = ResNetSimple_decoder(2, True)
        self.dense_center = False

    def center_features(self, x0, ind, chain=False):
        """center_feat_up0 -> center_feat_up1 -> gather at the 2 centre pixels (:790-792).
        sparse (default): exact evaluation on the 5x5 window of x0 around each centre -- up0 on the 3x3
        neighbourhood (zeroed where it leaves the map, because up1's padding pads up0 with zeros), then up1
        at the centre: 0.06 instead of 48.3 GFLOP/img, same values.
        dense: the reference formulation (two full 3x3 convolutions, then keep 2 pixels)."""
        if self.dense_center:
            out = F.gather_rows(self.center_feat_up1(self.center_feat_up0(x0)), ind)
            return (out, x0) if chain else out
        B, _, H, W = x0.shape
        up0, up1 = self.center_feat_up0, self.center_feat_up1
        win = F.window_gather(x0, ind, 2, chain)                                           # [B*2,256,5,5]
        if chain:
            win, x0_next = win
        u0 = F.conv2d(win, up0.weight, None, 1, 0)                                         # [B*2,512,3,3] (valid conv)
        u0 = F.window_mask(u0, ind, H, W, 1)
        # a valid 3x3 convolution of a 3x3 map is one full contraction: a plain [B*2, 9*512] x [1024, 9*512]^T GEMM on the NHWC
        # rows (as a convolution the backward-data pass walks 9 taps of which 8 are masked per position)
        u1 = F.linear(u0.permute(0, 2, 3, 1).reshape(B * 2, -1), F.as_matrix(up1.weight))  # [B*2,1024]
        return (u1.reshape(B, 2, 1024), x0_next) if chain else u1.reshape(B, 2, 1024)

    def forward(self, img, ind, choose, cloud, depth=None, K_new=None, valid=None):
        """The reference's encoder call (intaghand_encoder.py:706-811): trunk and dense branches in one go."""
        st = self.trunk(img, ind, choose, cloud, depth, K_new, valid)
        hms, mask, ret, hms_f, dp_f = self.dense_branches(st)
        return hms, mask, ret, st['img_fmaps'], hms_f, dp_f, st['ind']

    def rgb_encoder(self, img):
        """BASELINE config 2: the RGB-only part of the encoder call (intaghand_encoder.py:711-744) -- e_conv1, the ResNet-50
        trunk, the pyramid laterals + L2Norm, cat -> feat -> feat_bn -> ReLU.
        Returns (x0 [B,256,R/4,R/4], emb0 [B,3,R,R], x1 [B,2048,R/32,R/32])."""
        r = self.resnet
        img = F.cl(img)
        emb0 = self.e_conv1(img, F.ACT_RELU)                                              # :711
        emb1 = r.bn1(r.conv1(img, stats=r.bn1.training), relu=True)                                             # :712-715
        x4 = r.layer1(F.maxpool3s2(emb1))
        x3 = r.layer2(x4)
        x2 = r.layer3(x3)
        x1 = r.layer4(x2)
        pyr = F.l2norm_cat([self.p2(x4), self.p3(x3), self.p4(x2), self.p5(x1)],         # NHWC channel concat, written in place
                           [self.p2_l2.weight, self.p3_l2.weight, self.p4_l2.weight, self.p5_l2.weight])
        return self.feat_bn(self.feat(pyr, stats=self.feat_bn.training), relu=True), emb0, x1     # :740-744

    def trunk_layers(self, pooled):
        """layer1..layer4 -> (x4, x3, x2, x1); under a Trainer replayed from a tape of its library calls (pdfnet_amd/taped.py): same launches,
        none of the Python between them."""
        seg = self.__dict__.get('_trunk_seg')
        if seg is None:
            from ..taped import TapedSegment
            r = self.resnet
            layers = [r.layer1, r.layer2, r.layer3, r.layer4]
            seg = self.__dict__['_trunk_seg'] = TapedSegment(layers, layers)
        return seg(pooled)

    def trunk(self, img, ind, choose, cloud, depth=None, K_new=None, valid=None):
        """Everything the mesh decoder waits on: ResNet, pyramid, `feat`, the centre heat-map head, centre features,
        PointNet++ per hand and the SFT fusion.  Returns a state dict for `dense_branches`."""
        r = self.resnet
        img = F.cl(img)
        emb0 = self.e_conv1(img, F.ACT_RELU)                                              # :711
        emb1 = r.bn1(r.conv1(img, stats=r.bn1.training), relu=True)                                             # :712-715
        have_clouds = choose is not None and cloud is not None
        f_pn = None
        # Feature maps with several scatter-type consumers (emb0 / emb1: both hands' row gathers, emb1 also the max pool; x0: the
        # centre windows and both hands' gathers) are handed from consumer to consumer (`chain`): their backward passes then fill
        # ONE gradient tensor per map -- no zero-filled 134 MB tensor per consumer, no add pass per pair (0.27 ms per step)
        chain = have_clouds and emb1.requires_grad
        pooled = F.maxpool3s2(emb1, skip=chain)
        emb1c = emb1
        if chain:
            pooled, emb1c = pooled
        if have_clouds:                                                                    # measured: 374 vs 348 img/s
            pn = self.pointnet_plus                                                        # left first: BN update order (:805-806)

            def both_hands():
                if not chain:
                    return pn.stage_a(cloud[:, 0], emb0, emb1, choose[:, 0]), pn.stage_a(cloud[:, 1], emb0, emb1, choose[:, 1])
                xl, yl, e0, e1 = pn.stage_a(cloud[:, 0], emb0, emb1c, choose[:, 0], True)
                xr, yr, _, _ = pn.stage_a(cloud[:, 1], e0, e1, choose[:, 1], True)
                return (xl, yl), (xr, yr)
            f_pn = F.fork(both_hands)
        x4, x3, x2, x1 = self.trunk_layers(pooled)
        if self.on_trunk_output_grad is not None and x1.requires_grad:
            # fires in the backward once d loss / d x1 is complete, i.e. when every branch above the trunk has run its backward
            cb = self.on_trunk_output_grad
            x1.register_hook(lambda g: cb())
        st = {'x1': x1, 'ret': {}}
        pyr = F.l2norm_cat([self.p2(x4), self.p3(x3), self.p4(x2), self.p5(x1)],         # NHWC channel concat, written in place
                           [self.p2_l2.weight, self.p3_l2.weight, self.p4_l2.weight, self.p5_l2.weight])
        x0 = self.feat_bn(self.feat(pyr, stats=self.feat_bn.training), relu=True)                 # :740-744
        F.share_winograd_input(x0)                  # hm / wh / params heads and center_feat_up0 all read x0: one input transform
        st['x0'] = x0
        hm_fc = self.hm
        st['ret']['hm'] = hm_fc[2](hm_fc[0](x0, F.ACT_RELU))                               # 'hm' is first in opt.heads (:291)
        if ind is None:                                                                    # :750-758
            ind = nms_top1_centers(st['ret']['hm'])
        chain0 = f_pn is not None and x0.requires_grad and not self.dense_center
        f_center = F.fork(lambda: self.center_features(x0, ind, chain0))                   # [B,2,1024]  (:790-792)
        x0c = f_center.out[1] if chain0 else x0                                            # (a view of x0: usable before the join)
        emb = [emb0, emb1, x0]
        if choose is None or cloud is None:
            # test/demo path (:779-784): clouds from the depth map and the PREDICTED hand masks -- on the GPU, any batch
            # size (the reference does this on the CPU with numpy, batch 1).  The reference triggers it with a host-side
            # `choose.sum() == 0`; here it is requested explicitly by passing choose=None (no device->host sync).
            if depth is None or K_new is None:
                raise ValueError("pdfnet_amd: choose/cloud are None, so depth and K_new are required to build the clouds")
            st['dp'] = self.dp_decoder(x1)
            if valid is None:
                valid = torch.ones((img.shape[0], 2), device=img.device)
            choose, cloud, _ = F.depth2pcl(depth, st['dp'][0], K_new, valid)
            if getattr(self.opt, 'sample_strategy', 'Random') == 'FPS':                   # lib/opts.py:231; interhand.py:857-900
                B_ = cloud.shape[0]
                c2, ch2 = F.fps_reorder(cloud.reshape(B_ * 2, 1024, 3), choose.reshape(B_ * 2, 1024), self.opt.sample_num_level1, self.opt.sample_num_level2)
                cloud, choose = c2.reshape(B_, 2, 1024, 3), ch2.reshape(B_, 2, 1024)
        if f_pn is not None:
            al, ar = f_pn.join()
            if chain0:
                fl, x0c = self.pointnet_plus.stage_b(*al, x0c, choose[:, 0], True)
                fr, _ = self.pointnet_plus.stage_b(*ar, x0c, choose[:, 1], True)
            else:
                fl = self.pointnet_plus.stage_b(*al, x0, choose[:, 0])
                fr = self.pointnet_plus.stage_b(*ar, x0, choose[:, 1])
        else:
            fl = self.pointnet_plus(cloud[:, 0], emb, choose[:, 0])                        # :805
            fr = self.pointnet_plus(cloud[:, 1], emb, choose[:, 1])                        # :806 (same module: left BN update first)
        center = f_center.join()
        if chain0:
            center = center[0]
        fuse = self.sft(torch.cat((fl, fr), 1), center)                                    # [B,2,1024]  (:807-809)
        st['img_fmaps'] = [fuse, x2, x3, x4]
        st['ind'] = ind
        return st

    def dense_branches(self, st, defer=False, lazy_heads=False):
        """The two up-sampling decoders (need only x1) and the wh / params heads (need only x0; no loss term): heavy
        convolutions with few launches, each on its own side stream, joined right away.  (Starting them as early as their
        inputs exist, next to the pyramid / feat convolutions, was measured: 346 vs 366 img/s -- MFMA-bound work gains
        nothing from running beside MFMA-bound work; only the HBM-bound PointNet++ levels are started early.)"""
        x0, x1 = st['x0'], st['x1']
        f_hms = F.fork(lambda: self.hms_decoder(x1))
        f_dp = F.fork(lambda: self.dp_decoder(x1)) if 'dp' not in st else None

        def other_heads():
            out = {}
            for head in self.opt.heads:
                if head != 'hm':
                    fc = getattr(self, head)
                    out[head] = fc[2](fc[0](x0, F.ACT_RELU))
            return out
        # lazy_heads (round 5, the trainer's switch): the wh / params heads carry no loss term (lib/trains/simplified.py:397-399), so nothing in the
        # step waits for them: `join` then returns their closure instead of their outputs, and the caller issues it AFTER the loss -- beside the
        # launch-bound start of the backward instead of beside the mesh decoder, where 0.9 ms of their convolutions widened the forward
        f_heads = None if lazy_heads else F.fork(other_heads)
        def join():
            ret = dict(st['ret'])
            for head in self.opt.heads:                                                    # keep the reference's key order
                if head != 'hm':
                    ret[head] = None
            if f_heads is not None:
                ret.update(f_heads.join())
            else:
                ret['_lazy_heads'] = other_heads
            hms, hms_f = f_hms.join()
            mask, dp_f = f_dp.join() if f_dp is not None else st['dp']
            return hms, mask, ret, hms_f, dp_f
        return join if defer else join()


class resnet_mid(nn.Module):
    """intaghand_encoder.py:822-881: conv1x1 -> ReLU -> BN on cat(hms_f, dp_f[, img_f]).  Its fmaps are
    only shape-asserted downstream (DualGraph.py:69-72) but its BN running statistics are live state."""

    def __init__(self, out_dims):
        super().__init__()
        self.convs = nn.ModuleList()
        for i, od in enumerate(out_dims):
            cin = 256 + (0 if i == 0 else [2048, 1024, 512, 256][i])
            bn = BatchNorm(od)
            self.convs.append(nn.Sequential(Conv2d(cin, od, 1, bias=False), Slot(), bn))
        self.global_feature_dim = 1024
        self.fmaps_dim = out_dims

    def get_info(self):
        return {'global_feature_dim': self.global_feature_dim, 'fmaps_dim': self.fmaps_dim}

    def forward(self, img_f, hms_f, dp_f):
        fmaps = []
        for i, conv in enumerate(self.convs):
            parts = [hms_f[i], dp_f[i]] + ([img_f[i]] if i > 0 else [])
            fmaps.append(conv[2](conv[0](torch.cat(parts, 1), F.ACT_RELU, stats=conv[2].training)))
        return img_f[0][:, 0], img_f[0][:, 1], fmaps


def load_encoder(opt):
    """intaghand_encoder.py:1064-1087."""
    return ResNetSimple(opt), resnet_mid(opt.DECONV_DIMS)
