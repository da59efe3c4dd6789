from .hmm_inference import hmm_estep_differentiable, hmm_estep_vjp, vjp_redone_sequences  # noqa: F401
from .hmm_inference import sample_redone_sequences  # noqa: F401
from .hmm_inference import hmm_viterbi_perstep, hmm_sample_perstep  # noqa: F401
from .hmm_inference import hmm_estep_perstep_differentiable, hmm_estep_perstep_vjp  # noqa: F401
from .hmm_inference import hmm_estep_chunked, hmm_logZ_chunked, chunked_redone_sequences  # noqa: F401
from .hmm_inference import hmm_viterbi_chunked, hmm_sample_chunked  # noqa: F401
