"""``bootstrap`` of the reference (analysis/bootstrap.py) -> thermompnn_amd."""
import _repo  # noqa: F401
from thermompnn_amd.bootstrap import bootstrap_metrics, bootstrap_metrics_host, main  # noqa: F401

if __name__ == "__main__":
    raise SystemExit(main())
