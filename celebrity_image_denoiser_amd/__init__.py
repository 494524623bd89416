"""MI355X-native forward of the reference's denoising U-Net (`DenoiseGenerator`).

Public surface (mirrors what the reference's callers use, reference backend/app.py:319-336,422-435):

    DenoiseGenerator()            nn.Module-protocol object: .to(), .load_state_dict(), .eval(), __call__
    load(path_or_state_dict)      -> DenoiseGenerator on the current GPU, weights loaded like load_state_safely
    denoise(model, image_batch)   -> image_batch
    denoise_u8(model, uint8 NHWC) -> uint8 NHWC (pre/post-processing fused into the first/last kernel)
    HostPipeline(model).run(host_batches)   upload / forward / download overlapped on three HIP streams
    GraphedForward(model, example)(x)       the forward at a fixed shape as one HIP-graph launch (N=1 serving latency)
    enhance_images(ckpt, in_dir, out_dir)   the reference's directory eval harnesses (denoisegan_eval.py / denoise_eavl_iter.py)
    quality(a, b) / evaluate(denoised, clean)   PSNR / SSIM / MS-SSIM of device batches (the trainer's per-batch evaluation)
    add_noise(clean_u8, kind)     the trainer's five noise kinds on device uint8 batches; evaluate_noise_types(model, clean_u8)
    resize(src_u8, (width, height)) / resize_images(list, size)   PIL's bicubic Image.resize on device uint8 batches, bit for bit
    DenoiseDiscriminator() / load_discriminator(ckpt)   the trainer's discriminator (eval or train-mode BatchNorm); with
                                  autograd=True its forward is differentiable (HIP backward pass): d_loss.backward() and the
                                  adversarial gradient on the denoised batch, for a stock torch.optim optimizer
    trainer_losses(D, denoised, clean)                  the trainer's d_loss / g_loss / content_loss / adv_loss of one batch
    SRGANDiscriminator() / load_srgan_discriminator(ckpt)   the SRGAN trainer's discriminator (eval or train-mode BatchNorm); with
                                  autograd=True its forward is differentiable (HIP backward pass), as DenoiseDiscriminator's;
                                  srgan_trainer_losses(D, fake_hr, hr_img, vgg_loss) -> its d_loss / adv_loss / g_loss
    Adam(params, lr, betas, eps, weight_decay)          the trainer's optimizer as one kernel per step (cid_adam_step); its state
                                  interchanges with torch.optim.Adam's
    ESRGANGenerator(num_residuals=8) / load_esrgan(ckpt)   the server's ESRGAN model (eval mode); enhance(model, x) -> the raw
                                  fp32 output, enhance_u8(model, u8) -> the server's uint8 view; with batch_stats=True a
                                  train-mode forward (batch-statistics BatchNorm under the blocks' skips): the ESRGAN trainer's G(noisy),
                                  with autograd=True as well a differentiable one (HIP backward pass): its g_loss.backward()
    SRGANGenerator(scale_factor=4) / load_srgan(ckpt)      the server's SRGAN model (eval mode): super_resolve(model, x) -> fp32 at
                                  scale times the size, super_resolve_u8(model, u8) -> the server's padded uint8 view; with
                                  batch_stats=True a train-mode forward (batch-statistics BatchNorm), with autograd=True as well a
                                  differentiable one (HIP backward pass): g_loss.backward() of the SRGAN trainer
    CGANGenerator(n_classes=10) / load_cgan(ckpt)          the server's class-conditional cGAN model (eval mode): latent(n, seed) draws
                                  its input on the device, generate(model, labels, seed=s) -> fp32 [N,3,64,64], generate_u8 -> the
                                  server's uint8 view
    LPIPS(net) / load_lpips(lin_ckpt, backbone, net=net)   lpips.LPIPS(net='alex'), the trainers' third metric, or net='vgg', the ESRGAN
                                  trainer's: metrics.lpips(a, b, model) -> float64 [N]; evaluate(denoised, clean, lpips=model) fills
                                  the third value
    ESRGANDiscriminator(input_shape) / load_esrgan_discriminator(ckpt)   the ESRGAN trainer's discriminator, forward only: fp32 logits
                                  [N,1]; esrgan_trainer_losses(D, denoised, clean) -> that trainer's d_loss, gan_loss, pixel_loss, g_loss
    VGGPerceptualLoss() / load_vgg_loss(backbone)          the SRGAN and denoise trainers' content loss, MSE of vgg16.features[:16];
                                  with autograd=True differentiable with respect to its first operand (HIP backward), else the
                                  value only, no autograd history

Everything numeric runs in hand-written HIP kernels behind the C ABI in include/cid.h
(csrc/ -> libcid.so).  There is no CPU fallback: if the library is missing the calls raise.
"""
__version__ = "0.1.0"

_LAZY = {
    "DenoiseGenerator": ("generator", "DenoiseGenerator"),
    "load": ("api", "load"),
    "denoise": ("api", "denoise"),
    "denoise_u8": ("api", "denoise_u8"),
    "serve_u8": ("api", "serve_u8"),
    "get_padding": ("api", "get_padding"),
    "load_state_safely": ("api", "load_state_safely"),
    "psnr": ("metrics", "psnr"),
    "quality": ("metrics", "quality"),
    "evaluate": ("metrics", "evaluate"),
    "NOISE_TYPES": ("noise", "NOISE_TYPES"),
    "add_noise": ("noise", "add_noise"),
    "evaluate_noise_types": ("noise", "evaluate_noise_types"),
    "resize": ("resize", "resize"),
    "resize_images": ("resize", "resize_images"),
    "DenoiseDiscriminator": ("discriminator", "DenoiseDiscriminator"),
    "load_discriminator": ("discriminator", "load_discriminator"),
    "trainer_losses": ("discriminator", "trainer_losses"),
    "SRGANDiscriminator": ("srgan_disc", "SRGANDiscriminator"),
    "load_srgan_discriminator": ("srgan_disc", "load_srgan_discriminator"),
    "srgan_trainer_losses": ("srgan_disc", "srgan_trainer_losses"),
    "ESRGANDiscriminator": ("esrgan_disc", "ESRGANDiscriminator"),
    "load_esrgan_discriminator": ("esrgan_disc", "load_esrgan_discriminator"),
    "esrgan_trainer_losses": ("esrgan_disc", "esrgan_trainer_losses"),
    "Adam": ("optim", "Adam"),
    "ESRGANGenerator": ("esrgan", "ESRGANGenerator"),
    "load_esrgan": ("esrgan", "load_esrgan"),
    "enhance": ("esrgan", "enhance"),
    "enhance_u8": ("esrgan", "enhance_u8"),
    "SRGANGenerator": ("srgan", "SRGANGenerator"),
    "load_srgan": ("srgan", "load_srgan"),
    "super_resolve": ("srgan", "super_resolve"),
    "super_resolve_u8": ("srgan", "super_resolve_u8"),
    "CGANGenerator": ("cgan", "CGANGenerator"),
    "load_cgan": ("cgan", "load_cgan"),
    "latent": ("cgan", "latent"),
    "generate": ("cgan", "generate"),
    "generate_u8": ("cgan", "generate_u8"),
    "LPIPS": ("lpips", "LPIPS"),
    "load_lpips": ("lpips", "load_lpips"),
    "VGGPerceptualLoss": ("lpips", "VGGPerceptualLoss"),
    "load_vgg_loss": ("lpips", "load_vgg_loss"),
    "HostPipeline": ("pipeline", "HostPipeline"),
    "denoise_host_batches": ("pipeline", "denoise_host_batches"),
    "GraphedForward": ("pipeline", "GraphedForward"),
    "enhance_images": ("harness", "enhance_images"),
}


def __getattr__(name):
    if name in _LAZY:
        import importlib

        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(__name__ + "." + mod), attr)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
