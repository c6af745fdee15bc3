"""Stage-3 slice of the reference's ``RefRestorationModel`` (ref_restoration_model.py:21-43, 47-87, 186-279): net
construction through the registry, the four Adam parameter groups, ``feed_data`` / ``optimize_parameters`` / ``test``.  The
losses: the pixel loss (the MSE yaml) and, where ``train.perceptual_opt`` is present, the perceptual loss of the GAN yaml
(mmsr/models/losses.py) with the reference's two phases (ref_restoration_model.py:199-269): up to
``train.net_g_pretrain_steps`` the pixel loss alone (log key ``l_pix``), afterwards pixel + perceptual (``l_g_pix``,
``l_g_percep``).  The loss module sits bare on the device: it has no trainable parameter, is never DDP-wrapped and never
enters a checkpoint.  Without ``perceptual_opt`` and ``network_d`` the step, its log key and the graph handling are what they
were.  ``style_opt``, ``texture_opt`` and the LR schedulers are not provided here -- ``mmsr/train.py`` of the reference keeps
using its own model file; this class is what bench/tests drive.

The critic (``network_d`` together with ``train.gan_type``; single process): ``net_d`` through the registry, its own Adam
(``lr_d``, ``weight_decay_d``, ``beta_d``) as the second entry of ``self.optimizers``, ``GANLoss`` and, with
``grad_penalty_weight > 0``, ``GradientPenaltyLoss``.  After the pretrain phase every step first trains the critic on
``D(gt)``, ``D(output.detach())`` and the penalty, then -- when ``(step - pretrain) % net_d_steps == 0`` and
``(step - pretrain) > net_d_init_steps`` -- the generator on pixel + perceptual + ``cri_gan(D(output), True)`` with the
critic's parameters frozen (ref_restoration_model.py:209-269).  Log keys in the reference's order: ``l_d_real``,
``out_d_real``, ``l_d_fake``, ``out_d_fake``, ``l_grad_penalty``, ``l_g_pix``, ``l_g_percep``, ``l_g_gan``, all device tensors.
The critic's BatchNorm layers run in train mode in each of its three or four forwards of a step, as in the reference.
``opt['dist']`` with a critic raises NotImplementedError.

Validation: ``nondist_validation`` computes PSNR / PSNR_Y / SSIM_Y with the reference's rules
(ref_restoration_model.py:295-370) but on the device: one kernel reads SR and GT once and leaves three sums per image and,
with ``save_img``, the uint8 image that is written as a PNG under the reference's path rules (c2m_amd.ops.val_metrics;
``C2M_VAL_FUSED=0`` and CPU tensors take the torch composition of mmsr/utils/metrics.py); ``dist_validation`` -- which in the reference calls a method that does not exist
(sr_model.py:160-162) -- shards the loader over the ranks and all-reduces the sums.

MI355X addition -- ``train: {hip_graph: true}`` (single-process training): the whole training step (extractor +
correspondence + net_g forward + L1 + backward + Adam) is a launch-bound chain of ~1500 small kernels at the reference's
stage-3 crop size (GT 160x160, batch 4 per GPU): the host spends more time launching than the GPU computing.  The step is
captured once into a hipGraph (torch.cuda.CUDAGraph: static input buffers filled by ``feed_data``, Adam in capturable
mode, two eager warm-up steps so that allocator, MIOpen find and lazy initialisation stay outside the capture) and
replayed per ``optimize_parameters`` call -- same arithmetic, same kernels, one launch.  With a perceptual loss each of the
two phases is its own captured step: crossing ``net_g_pretrain_steps`` drops the graph, and the next calls warm up and capture
again, as after a new input geometry.  With a critic only the pretrain phase is captured: the GAN phase
(``autograd.grad(create_graph=True)``, a second optimizer) runs eagerly.
"""
import collections
import copy
import logging
import os

import torch

import mmsr.models.networks as networks
from mmsr.models.base_model import BaseModel, unwrap
from mmsr.utils import metrics

logger = logging.getLogger('base')

# C2M_VAL_FUSED (default 1): validation metrics and the saved image of fp32 tensors on the GPU by the one-pass kernel
# (c2m_amd.ops.val_metrics); 0: the torch composition metrics.validation_metrics.  Read once, like the other switches.
_VAL_FUSED = os.environ.get("C2M_VAL_FUSED", "1") != "0"


class RefRestorationModel(BaseModel):

    def __init__(self, opt):
        super().__init__(opt)
        with_critic = bool(self.is_train and opt.get('network_d') and (opt.get('train') or {}).get('gan_type'))
        if with_critic and opt.get('dist'):
            raise NotImplementedError("network_d with opt['dist']: the critic's three forwards before one backward and the "
                                      "penalty's autograd.grad are not wired for DistributedDataParallel; train the GAN "
                                      "phase in a single process")
        opt = copy.deepcopy(opt)  # the factories pop 'type'
        self.net_g = self.model_to_device(networks.define_net_g(opt))
        # net_map has no trainable parameters; net_extractor's never receive gradients in stage 3: both stay bare
        self.net_map = self.model_to_device(networks.define_net_map(opt), receives_gradients=False)
        self.net_extractor = self.model_to_device(networks.define_net_extractor(opt), receives_gradients=False)
        for p in self.net_extractor.parameters():
            p.requires_grad = False
        path = self.opt.get('path') or {}
        if path.get('pretrain_model_feature_extractor'):
            self.load_network(self.net_extractor, path['pretrain_model_feature_extractor'], path.get('strict_load', True))
        if path.get('pretrain_model_g'):
            self.load_network(self.net_g, path['pretrain_model_g'], path.get('strict_load', True))
        # (one process, ONE device: nn.DataParallel's scatter / replicate / worker threads cannot be captured)
        self._graph_on = bool(self.is_train and (self.opt.get('train') or {}).get('hip_graph') and not self.opt.get('dist')
                              and self.device.type == 'cuda' and not isinstance(self.net_g, torch.nn.DataParallel))
        if self._graph_on:
            # the captured step cannot read the f16 x 2 range flag back (c2m_amd.ops.f16_range_guard): the frozen nets that run
            # under no_grad inside it keep the full-range bf16 x 3 flavour from the first (eager) step on
            for net in (self.net_extractor, self.net_map):
                for m in net.modules():
                    m._c2m_conv_bf16x3 = True
        self._eval_feed = False   # True while a validation loop feeds data: its batches bypass the graph's static buffers
        self._graph, self._graph_calls, self._static = None, 0, None
        if self.is_train:
            self.net_g.train()
            self._build_optimizer()
            self.cri_pix = torch.nn.L1Loss()  # pixel_criterion: L1Loss, pixel_weight 1.0 (stage3_restoration_mse.yml:84-85)
            self.pixel_weight = float(self.opt['train'].get('pixel_weight', 1.0))
            # the GAN yaml's perceptual_opt (ref_restoration_model.py:119-125, :165); absent: the pixel-loss step as it was
            self.cri_perceptual = None
            self.net_g_pretrain_steps = int(self.opt['train'].get('net_g_pretrain_steps') or 0)
            self._pretrain = False    # the phase of the step being run / captured
            if self.opt['train'].get('perceptual_opt'):
                from mmsr.models.losses import PerceptualLoss
                self.cri_perceptual = PerceptualLoss(**self.opt['train']['perceptual_opt']).to(self.device)
            # the GAN yaml's network_d / gan_type block (ref_restoration_model.py:92-107, :143-179); absent: nothing changes
            self.net_d = self.cri_gan = self.cri_grad_penalty = None
            if with_critic:
                self._build_critic(opt, path)
            self._phased = self.cri_perceptual is not None or self.net_d is not None

    def _build_optimizer(self):
        """Adam with the reference's four groups keyed on parameter names (ref_restoration_model.py:47-87)."""
        t = self.opt['train']
        groups = {'g': [], 'offset': [], 'relu3_offset': [], 'relu2_offset': []}
        for name, p in unwrap(self.net_g).named_parameters():
            if not p.requires_grad:
                continue
            if 'offset' in name:
                key = 'relu3_offset' if 'small' in name else 'relu2_offset' if 'medium' in name else 'offset'
            else:
                key = 'g'
            groups[key].append(p)
        self.optimizer_g = torch.optim.Adam(
            [{'params': groups['g']},
             {'params': groups['offset'], 'lr': t['lr_offset']},
             {'params': groups['relu3_offset'], 'lr': t['lr_relu3_offset']},
             {'params': groups['relu2_offset'], 'lr': t['lr_relu2_offset']}],
            lr=t['lr_g'], weight_decay=t.get('weight_decay_g', 0), betas=tuple(t['beta_g']),
            capturable=self._graph_on)   # (step counters on the device: required inside a captured step)
        self.optimizers.append(self.optimizer_g)

    def _build_critic(self, opt, path):
        from mmsr.models.losses import GANLoss, GradientPenaltyLoss
        t = self.opt['train']
        self.net_d = self.model_to_device(networks.define_net_d(opt))
        if path.get('pretrain_model_d'):
            self.load_network(self.net_d, path['pretrain_model_d'], path.get('strict_load', True))
        self.net_d.train()
        self.cri_gan = GANLoss(t['gan_type'], real_label_val=1.0, fake_label_val=0.0, loss_weight=t['gan_weight']).to(self.device)
        if (t.get('grad_penalty_weight') or 0) > 0:
            self.cri_grad_penalty = GradientPenaltyLoss(loss_weight=t['grad_penalty_weight']).to(self.device)
        self.net_d_steps = int(t.get('net_d_steps') or 1)
        self.net_d_init_steps = int(t.get('net_d_init_steps') or 0)
        self._step = 0
        self._gan_eager_logged = False
        self.optimizer_d = torch.optim.Adam(self.net_d.parameters(), lr=t['lr_d'], weight_decay=t.get('weight_decay_d', 0),
                                            betas=tuple(t['beta_d']))
        self.optimizers.append(self.optimizer_d)   # save_training_state / resume_training carry it

    _FEED = (('img_in_lq', 'img_in_lq'), ('img_ref', 'img_ref'), ('gt', 'img_in'), ('match_img_in', 'img_in_up'))

    def feed_data(self, data):
        if self._graph_on and not self._eval_feed:
            # static input buffers: the captured step reads these addresses; a new batch is copied INTO them
            shapes = {a: tuple(data[k].shape) for a, k in self._FEED}
            if self._static is None or {a: tuple(t.shape) for a, t in self._static.items()} != shapes:
                self._static = {a: data[k].to(self.device, copy=True) for a, k in self._FEED}
                self._graph, self._graph_calls = None, 0    # new geometry: capture again
            else:
                for a, k in self._FEED:
                    self._static[a].copy_(data[k], non_blocking=True)
            for a, _ in self._FEED:
                setattr(self, a, self._static[a])
            return
        self.img_in_lq = data['img_in_lq'].to(self.device)
        self.img_ref = data['img_ref'].to(self.device)
        self.gt = data['img_in'].to(self.device)
        self.match_img_in = data['img_in_up'].to(self.device)

    def _correspondence(self):
        with torch.no_grad():  # non-differentiable past the arg-max; keeps DDP's reducer to net_g only
            self.features = self.net_extractor(self.match_img_in, self.img_ref)
            self.pre_offset, self.img_ref_feat = self.net_map(self.features, self.img_ref)

    def optimize_parameters(self, step):
        if self._phased:
            pretrain = step <= self.net_g_pretrain_steps
            if pretrain != self._pretrain:
                self._pretrain = pretrain
                self._graph, self._graph_calls = None, 0    # the other phase is another step: warm up and capture again
                self.log_dict.clear()
        if self.net_d is not None:
            self._step = step
            if self._graph_on and not self._pretrain:
                # autograd.grad(create_graph=True) and a second optimizer inside a capture are untried: the GAN phase is eager
                if not self._gan_eager_logged:
                    logger.info('hip_graph: the GAN phase (critic + gradient penalty) runs eagerly; only the pretrain phase '
                                'is captured.')
                    self._gan_eager_logged = True
                return self._train_step()
        if self._graph_on:
            return self._optimize_graphed()
        self._train_step()

    def _train_step(self):
        self._correspondence()
        self.output = self.net_g(self.img_in_lq, self.pre_offset, self.img_ref_feat)
        self.optimizer_g.zero_grad()
        l_pix = self.cri_pix(self.output, self.gt) * self.pixel_weight
        if self._phased:
            return self._perceptual_step(l_pix)
        l_pix.backward()  # DCNv2 backward x3; DDP all-reduces net_g's gradients (RCCL) while it runs
        self.optimizer_g.step()
        self.log_dict['l_g_pix'] = l_pix.detach()  # no .item(): the reference's per-step host sync is dropped

    def _perceptual_step(self, l_pix):
        """The rest of a step of the GAN yaml (ref_restoration_model.py:199-269): the pretrain step, or the critic's step (with a
        critic) followed by the generator's where the step gating allows it; the log values stay device tensors and nothing is
        read back."""
        if self._pretrain:
            l_pix.backward()
            self.optimizer_g.step()
            self.log_dict['l_pix'] = l_pix.detach()
            return
        if self.net_d is not None:
            self._critic_step()
            k = self._step - self.net_g_pretrain_steps
            if k % self.net_d_steps != 0 or k <= self.net_d_init_steps:
                return
        l_g_total = l_pix
        l_g_percep = None
        if self.cri_perceptual is not None:
            l_g_percep, _ = self.cri_perceptual(self.output, self.gt)   # (None with perceptual_weight 0, as in the reference)
        if l_g_percep is not None:
            l_g_total = l_g_total + l_g_percep
        l_g_gan = None
        if self.net_d is not None:
            # the critic is a fixed function in the generator's step: no gradient buffers for its parameters
            params_d = list(self.net_d.parameters())
            for p in params_d:
                p.requires_grad = False
            try:
                l_g_gan = self.cri_gan(self.net_d(self.output), True, is_disc=False)
                l_g_total = l_g_total + l_g_gan
                l_g_total.backward()
            finally:
                for p in params_d:
                    p.requires_grad = True
        else:
            l_g_total.backward()
        self.optimizer_g.step()
        self.log_dict['l_g_pix'] = l_pix.detach()
        if l_g_percep is not None:
            self.log_dict['l_g_percep'] = l_g_percep.detach()
        if l_g_gan is not None:
            self.log_dict['l_g_gan'] = l_g_gan.detach()

    def _critic_step(self):
        """One update of the critic on D(gt), D(output.detach()) and the gradient penalty (ref_restoration_model.py:209-232).
        The penalty gets the detached output: the critic's backward must not free the generator's graph, which the generator's
        step still needs, and no gradient reaches the generator through the penalty in the reference either."""
        self.optimizer_d.zero_grad()
        fake = self.output.detach()
        real_d_pred = self.net_d(self.gt)
        l_d_real = self.cri_gan(real_d_pred, True, is_disc=True)
        fake_d_pred = self.net_d(fake)
        l_d_fake = self.cri_gan(fake_d_pred, False, is_disc=True)
        l_d_total = l_d_real + l_d_fake
        l_grad_penalty = None
        if self.cri_grad_penalty is not None:
            l_grad_penalty = self.cri_grad_penalty(self.net_d, self.gt, fake)
            l_d_total = l_d_total + l_grad_penalty
        l_d_total.backward()
        self.optimizer_d.step()
        self.log_dict['l_d_real'] = l_d_real.detach()
        self.log_dict['out_d_real'] = real_d_pred.detach().mean()
        self.log_dict['l_d_fake'] = l_d_fake.detach()
        self.log_dict['out_d_fake'] = fake_d_pred.detach().mean()
        if l_grad_penalty is not None:
            self.log_dict['l_grad_penalty'] = l_grad_penalty.detach()

    GRAPH_WARMUP_STEPS = 2

    def _optimize_graphed(self):
        """Every call is exactly one training step: the first GRAPH_WARMUP_STEPS run eagerly on a side stream, the next one
        captures the step and replays it once, later ones only replay.  log_dict / output / the parameters' .grad keep
        their addresses: each replay rewrites them in place."""
        if self._graph is not None:
            self._graph.replay()
            self.output = self._graph_output   # (a validation in between re-pointed / deleted the attribute: ADVICE r4)
            return
        self._graph_calls += 1
        cur = torch.cuda.current_stream()
        if self._graph_calls <= self.GRAPH_WARMUP_STEPS:
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._train_step()
            cur.wait_stream(side)
            return
        self.optimizer_g.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._train_step()
        self._graph = graph
        self._graph_output = self.output       # the tensor every replay rewrites in place
        graph.replay()

    def save(self, epoch, current_iter):
        """net_g, net_d when there is one, and the training state (ref_restoration_model.py:289-293)."""
        self.save_network(self.net_g, 'net_g', current_iter)
        if getattr(self, 'net_d', None) is not None:
            self.save_network(self.net_d, 'net_d', current_iter)
        self.save_training_state(epoch, current_iter)

    # ---------------------------------------------------------------- validation
    def get_current_visuals(self):
        """The reference's dict of host tensors (ref_restoration_model.py:281-287): 'img_in_lq', 'rlt' and, when fed, 'gt'."""
        shown = [('img_in_lq', self.img_in_lq), ('rlt', self.output)] + ([('gt', self.gt)] if hasattr(self, 'gt') else [])
        return collections.OrderedDict((k, t.detach().cpu()) for k, t in shown)

    def _save_img_path(self, img_name, dataset_name, current_iter):
        """Where the reference writes a validation image (ref_restoration_model.py:317-329): while training
        <visualization>/<image>/<image>_<iter>.png, in a test run <visualization>/<dataset>/<image>_<name>[_<suffix>].png."""
        root = (self.opt.get('path') or {}).get('visualization')
        if not root:
            raise ValueError("save_img needs opt['path']['visualization'] (the directory the images go to)")
        if self.opt.get('is_train'):
            return os.path.join(root, img_name, f'{img_name}_{current_iter}.png')
        stem = f"{img_name}_{self.opt.get('name')}"
        if self.opt.get('suffix'):
            stem += f"_{self.opt['suffix']}"
        return os.path.join(root, dataset_name, stem + '.png')

    @staticmethod
    def _img_names(val_data, idx, count):
        """One name per item of the batch: the stem of its lq_path, or the loader index where the dict brings no paths."""
        paths = val_data.get('lq_path')
        if isinstance(paths, str):
            paths = [paths]
        names = [os.path.splitext(os.path.basename(p_))[0] for p_ in (paths or [])][:count]
        for b in range(len(names), count):
            names.append(str(idx) if count == 1 else f'{idx}_{b}')
        return names

    @staticmethod
    def _write_png(rgb_u8, path):
        """rgb_u8: uint8 [h, w, 3] host tensor, R G B."""
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("save_img=True writes PNG files with Pillow, which is not installed "
                               "(pip install pillow), or validate with save_img=False") from e
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(rgb_u8.contiguous().numpy(), 'RGB').save(path)

    @staticmethod
    def _fused_validation(sr, gt):
        """The one-pass kernel takes fp32 tensors on the GPU (unless C2M_VAL_FUSED=0); everything else the torch composition."""
        return bool(_VAL_FUSED and sr.is_cuda and gt.is_cuda and sr.dtype == torch.float32 and gt.dtype == torch.float32)

    def _validate_shard(self, dataloader, rank, world, save=None):
        """-> float64 tensor [psnr_sum, psnr_y_sum, ssim_y_sum, count] over items idx % world == rank.
        save: None, or (dataset name, current_iter): the SR image of every item of the shard is written as a PNG."""
        crop = self.opt.get('crop_border')
        crop = self.opt.get('scale', 4) if crop is None else crop   # options.py:56-57
        sums = torch.zeros(4, dtype=torch.float64, device=self.device)
        for idx, val_data in enumerate(dataloader):
            if idx % world != rank:
                continue
            self._eval_feed = True    # (differently shaped validation pairs must not reset the captured training step)
            try:
                self.feed_data(val_data)
            finally:
                self._eval_feed = False
            sr = self.test()
            gt = self.gt
            valid = None
            if val_data.get('padding', False) is not False and bool(torch.as_tensor(val_data['padding']).any()):
                # the reference crops only the SR image (:311-315); shapes must then agree
                valid = tuple(int(torch.as_tensor(v).flatten()[0]) for v in val_data['original_size'][:2])
            if self._fused_validation(sr, gt):
                # one pass over the padded tensors: the kernel reads the valid window only
                m = metrics.validation_metrics_fused(sr, gt, crop_border=crop, valid_hw=valid, images='rgb' if save else None)
                rgb = m['sr_u8'] if save else None
            else:
                if valid is not None:
                    sr, gt = sr[..., :valid[0], :valid[1]], gt[..., :valid[0], :valid[1]]
                with metrics.true_scalar_division():   # on the GPU too the composition divides by 255 as the reference does
                    m = metrics.validation_metrics(sr, gt, crop_border=crop)
                rgb = metrics.tensor2img_device(sr).flip(-1).to(torch.uint8) if save else None
            if save:
                rgb = rgb.cpu()
                for b, img_name in enumerate(self._img_names(val_data, idx, rgb.shape[0])):
                    self._write_png(rgb[b], self._save_img_path(img_name, save[0], save[1]))
            sums[0] += m['psnr'].sum()
            sums[1] += m['psnr_y'].sum()
            sums[2] += m['ssim_y'].sum()
            sums[3] += sr.shape[0]
            del self.img_in_lq, self.output, self.gt   # as the reference: keep peak memory at one batch (:331-335)
        return sums

    def _report(self, sums, name, current_iter, tb_logger):
        n = max(float(sums[3]), 1.0)
        res = {'psnr': float(sums[0]) / n, 'psnr_y': float(sums[1]) / n, 'ssim_y': float(sums[2]) / n, 'count': int(sums[3])}
        if self.rank <= 0:
            logger.info(f"# Validation {name} # PSNR: {res['psnr']:.4e} # PSNR_Y: {res['psnr_y']:.4e} "
                        f"# SSIM_Y: {res['ssim_y']:.4e}.")
            if tb_logger:
                for k in ('psnr', 'psnr_y', 'ssim_y'):
                    tb_logger.add_scalar(k, res[k], current_iter)
        return res

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        name = getattr(getattr(dataloader, 'dataset', None), 'opt', {}).get('name', 'val')
        sums = self._validate_shard(dataloader, 0, 1, save=(name, current_iter) if save_img else None)
        return self._report(sums, name, current_iter, tb_logger)

    def dist_validation(self, dataloader, current_iter, tb_logger, save_img):
        """Every rank validates its share of the loader; one all-reduce (RCCL on the GPU, gloo in the CPU tests) of four
        float64 sums gives every rank the dataset averages.  With save_img every rank writes the images of its own share."""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        name = getattr(getattr(dataloader, 'dataset', None), 'opt', {}).get('name', 'val')
        sums = self._validate_shard(dataloader, rank, world, save=(name, current_iter) if save_img else None)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        return self._report(sums, name, current_iter, tb_logger)

    def test(self):
        self.net_g.eval()
        with torch.no_grad():
            def whole():
                if self.img_ref.is_cuda:
                    # read the Ref's live extent while the queue is still empty; extractor and VGG taps share it
                    from c2m_amd import ops as _ops
                    _ops.ref_live_extent_shared(self.img_ref)
                self._correspondence()
                return self.net_g(self.img_in_lq, self.pre_offset, self.img_ref_feat)
            if self.img_in_lq.is_cuda:
                # ONE f16 x 2 range check for the whole inference step (extractor, VGG taps, RestorationNet): the module
                # forwards' own guards nest inside it and skip their read-backs -- one 4-byte device-to-host sync per step
                # instead of three (each one drains the GPU queue: ~0.3 ms of a 139 ms configs[2] step).  On overflow the whole
                # step is recomputed on the full-range flavour and this model keeps it (ops.f16_range_guard).
                from c2m_amd import ops as _ops
                self.output = _ops.f16_range_guard(self, whole, self.img_in_lq.device)
            else:
                self.output = whole()
        if self.is_train:
            self.net_g.train()
        return self.output
