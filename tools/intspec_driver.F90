! Driver of tools/make_golden_nest.py: calls the reference's INTSPEC (with its ROTSPEC and STRSPEC) on the cases of a stream file and writes
! what it returns.  It is built by oracle/ref_build.py::build_driver: the three routines, PARKIND_WAVE and YOWPCONS are the reference's own
! files, compiled unmodified in both precisions; the driver holds no module of its own.  The program sets ZPI of YOWPCONS as the model does
! (2 PI, PI = 4 ATAN(1)).
! Input  (stream, little endian): NCASE, NANG, NFRE (int32); FR(NFRE) (real64); per case DEL1L, FMEAN1, EMEAN1, THETM1, FMEAN2, EMEAN2,
!        THETM2 (real64), F1(NANG,NFRE), F2(NANG,NFRE) (real64).  Every value is representable in the working precision.
! Output (stream): per case FMEAN, EMEAN, THETM (real64), FL(NANG,NFRE) (real64): the working-precision results, widened.
PROGRAM INTSPEC_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWPCONS, ONLY : ZPI
  IMPLICIT NONE
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER(KIND=JWIM) :: NCASE, NANG, NFRE, IC
  REAL(KIND=R8) :: S(7)
  REAL(KIND=R8), ALLOCATABLE :: FR8(:), A8(:,:), B8(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: FR(:), F1(:,:), F2(:,:), FL(:,:)
  REAL(KIND=JWRB) :: FMEAN, EMEAN, THETM
  CHARACTER(LEN=512) :: FIN, FOUT

  ZPI = 8.0_JWRB*ATAN(1.0_JWRB)
  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) NCASE, NANG, NFRE
  ALLOCATE(FR8(NFRE), A8(NANG,NFRE), B8(NANG,NFRE), FR(NFRE), F1(NANG,NFRE), F2(NANG,NFRE), FL(NANG,NFRE))
  READ(11) FR8
  FR = REAL(FR8, JWRB)
  DO IC = 1, NCASE
    READ(11) S, A8, B8
    F1 = REAL(A8, JWRB)
    F2 = REAL(B8, JWRB)
    CALL INTSPEC(NFRE, NANG, NFRE, NANG, FR, 1.0_JWRB, REAL(S(1), JWRB),                    &
 &               F1, REAL(S(2), JWRB), REAL(S(3), JWRB), REAL(S(4), JWRB),                  &
 &               F2, REAL(S(5), JWRB), REAL(S(6), JWRB), REAL(S(7), JWRB),                  &
 &               FL, FMEAN, EMEAN, THETM)
    WRITE(12) REAL(FMEAN, R8), REAL(EMEAN, R8), REAL(THETM, R8), REAL(FL, R8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM INTSPEC_DRIVER
