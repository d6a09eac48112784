"""Command-line options of the extension.  A1111 calls preload(parser) for every extension before it parses the command line."""


def preload(parser):
    parser.add_argument(
        "--mdtile-devices", type=str, default=None,
        help="Tiled VAE on several GPUs of this process: comma-separated CUDA indices (a device may be listed more than once), or 'all'. "
             "The VAE's own device is always the first; the others need peer access to it. Default: the VAE's device only.")
