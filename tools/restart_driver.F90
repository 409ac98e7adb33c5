! Driver of tools/make_golden_restart.py: calls the reference's CDUSTARZ0, CHNKMIN, WRITEFL, WRITESTRESS and READSTRESS.  It is built by
! oracle/ref_build.py::build_driver: the routines and the modules they use are the reference's own files, compiled unmodified in both precisions,
! behind the stand-ins of oracle/ref_stubs.F90 for what other packages supply.  The program fills the run-time values of YOWPCONS, YOWPHYS and
! YOWWIND from its input and compares what the reference declares a PARAMETER; it holds no module of its own.
! BUILDSTRESS, READWGRIB, SAVSTRESS and GETSTRESS are bound to files and to the message passing library, so their statements on the fields
! (buildstress.F90:236-242, 279-313; readwgrib.F90:165-175; savstress.F90:112-127; getstress.F90:95-97, 150-165, 294-303) are restated here around
! the reference's routines.  IWAM_GET_UNIT is a stand-in that opens the file as the reference's does, but in the byte order of the machine: the
! reference's own asks for CONVERT='BIG_ENDIAN', and the restart layer of this project (ecwam_amd/restart.py, ECWAM_HIP_READFL / _WRITEFL) has always
! read and written the native order.  The records and their framing are those of the reference's WRITE statements.
! Input  (stream, little endian): N, NANG, NFRE, NCELL (int32); MAPIN(N), PERM(N) (int32, 1-based); WSPMIN, CDMAX, EPSUS, EPSU10, XKAPPA, RNUM, ALPHA,
!        ALPHAMIN, CHNKMIN_U, GM1, G, ZMISS, PRCHAR (real64, values of the working precision); FF(16,N), UWAVE(NCELL), CD(NCELL) (real64); NCASE (int32),
!        then per case LLCAPCHNK, HASCD, HASUWAVE, LNSESTART (int32), ZREF (real64); FL(NFRE,NANG,N), FFR(16,N), UCUR(N), VCUR(N) (real64); four dates
!        CHARACTER(14); ND (int32), DEPTH(ND), GAM_B_J (real64).  The third argument is the directory the four files BLS_ll1d, BLS_relab, LAW_ll1d, LAW_relab are written to.
! Output (stream): per case FF(16,N), CD(N), the branch code (N), real64; then what READSTRESS returned from LAW_ll1d and from LAW_relab, RFIELD(N,16)
!        each, real64; EMAXDPT(ND), real64.
PROGRAM RESTART_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWPCONS, ONLY : CDMAX, EPSUS, EPSU10, G
  USE YOWPHYS, ONLY : XKAPPA, RNUM, ALPHA, ALPHAMIN, CHNKMIN_U
  USE YOWWIND, ONLY : WSPMIN, CDAWIFL, CDATEWO, CDATEFL
  USE YOWSTAT, ONLY : CDTPRO
  USE YOWMPP, ONLY : NPROC
  USE YOWPARAM, ONLY : LL1D, LLUNSTR
  USE YOWSPEC, ONLY : IJ2NEWIJ
  IMPLICIT NONE
#include "chnkmin.intfb.h"
  INTEGER, PARAMETER :: NREAL = 16
  INTEGER, PARAMETER :: BR_UWAVE = 1, BR_CD = 2, BR_WSPMIN = 4, BR_Z0MIN = 8, BR_EPSUS = 16, BR_FLOOR_Z0M = 32, BR_TAUW0 = 64
  CHARACTER(LEN=512) :: FIN, FOUT, DIR
  CHARACTER(LEN=296) :: FILENAME
  INTEGER(KIND=JWIM) :: N, NANG, NFRE, NCELL, NCASE, ICASE, LLCAP, HASCD, HASUW, NSE, IJ, K, M, IUNIT, IPASS
  INTEGER(KIND=JWIM), ALLOCATABLE :: MAPIN(:), PERM(:), BR(:)
  REAL(KIND=8) :: R8(13), ZREF8
  REAL(KIND=8), ALLOCATABLE :: FF8(:,:), P8(:), FL8(:,:,:), V8(:)
  REAL(KIND=JWRB) :: ZMISS, PRCHAR, TEMPXNLEV, GM1, USTAR, CDSQRTINV, Z0TOT, CHARNOCKOG, ZA, ZB
  REAL(KIND=JWRB), ALLOCATABLE :: FF0(:,:), UWAVE(:), CDIN(:), FL(:,:,:), RFIELD(:,:), RBACK(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: WSWAVE(:), WDWAVE(:), UFRIC(:), TAUW(:), TAUWDIR(:), Z0M(:), Z0B(:), CHRNCK(:), CD(:), ALPHAOG(:), FFO(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: FFR(:,:), UCUR(:), VCUR(:), DEPTH(:), EMAXDPT(:)
  REAL(KIND=8), ALLOCATABLE :: D8(:)
  REAL(KIND=JWRB) :: GAM, GAM_B_J
  INTEGER(KIND=JWIM) :: ND
  ! the columns of FF, 1-based (include/ecwam_hip.h)
  INTEGER, PARAMETER :: JAIRD = 1, JWDWAVE = 2, JCICOVER = 3, JWSWAVE = 4, JWSTAR = 5, JUSTRA = 6, JVSTRA = 7, JUFRIC = 8, JTAUW = 9, JTAUWDIR = 10, &
 &                      JZ0M = 11, JZ0B = 12, JCHRNCK = 13, JCITHICK = 14

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  CALL GET_COMMAND_ARGUMENT(3, DIR)
  OPEN(10, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(11, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(10) N, NANG, NFRE, NCELL
  ALLOCATE(MAPIN(N), PERM(N), BR(N), FF8(16,N), P8(NCELL), FL8(NFRE,NANG,N), V8(N))
  ALLOCATE(FF0(16,N), UWAVE(NCELL), CDIN(NCELL), FL(N,NANG,NFRE), RFIELD(N,NREAL), RBACK(N,NREAL), FFO(16,N), FFR(16,N), UCUR(N), VCUR(N))
  ALLOCATE(WSWAVE(N), WDWAVE(N), UFRIC(N), TAUW(N), TAUWDIR(N), Z0M(N), Z0B(N), CHRNCK(N), CD(N), ALPHAOG(N))
  READ(10) MAPIN, PERM
  READ(10) R8
  WSPMIN = REAL(R8(1), JWRB)
  IF (REAL(R8(2), JWRB) /= CDMAX) ERROR STOP 'CDMAX'
  IF (REAL(R8(3), JWRB) /= EPSUS) ERROR STOP 'EPSUS'
  IF (REAL(R8(4), JWRB) /= EPSU10) ERROR STOP 'EPSU10'
  IF (REAL(R8(5), JWRB) /= XKAPPA) ERROR STOP 'XKAPPA'
  RNUM = REAL(R8(6), JWRB)
  ALPHA = REAL(R8(7), JWRB)
  ALPHAMIN = REAL(R8(8), JWRB)
  CHNKMIN_U = REAL(R8(9), JWRB)
  GM1 = REAL(R8(10), JWRB)
  G = REAL(R8(11), JWRB)
  ZMISS = REAL(R8(12), JWRB)
  PRCHAR = REAL(R8(13), JWRB)
  LLUNSTR = .FALSE.
  READ(10) FF8
  FF0 = REAL(FF8, JWRB)
  READ(10) P8
  UWAVE = REAL(P8, JWRB)
  READ(10) P8
  CDIN = REAL(P8, JWRB)
  READ(10) NCASE
  DO ICASE = 1, NCASE
    READ(10) LLCAP, HASCD, HASUW, NSE
    READ(10) ZREF8
    TEMPXNLEV = REAL(ZREF8, JWRB)
    FFO = FF0
    WSWAVE = FF0(JWSWAVE,:)
    WDWAVE = FF0(JWDWAVE,:)
    UFRIC = FF0(JUFRIC,:)
    TAUW = FF0(JTAUW,:)
    TAUWDIR = FF0(JTAUWDIR,:)
    Z0M = FF0(JZ0M,:)
    CHRNCK = FF0(JCHRNCK,:)
    BR = 0
    ! getstress.F90:95-97
    Z0B(:) = 0.0_JWRB
    ! READWGRIB's block step with LLONLYPOS (readwgrib.F90:165-175), restated
    IF (HASUW /= 0) THEN
      DO IJ = 1, N
        IF (UWAVE(MAPIN(IJ)) /= ZMISS .AND. UWAVE(MAPIN(IJ)) > 0.0_JWRB) THEN
          WSWAVE(IJ) = UWAVE(MAPIN(IJ))
          BR(IJ) = IOR(BR(IJ), BR_UWAVE)
        ENDIF
      ENDDO
    ENDIF
    ! buildstress.F90:236-242: the reference's CDUSTARZ0, then its two statements
    CALL CDUSTARZ0 (1, N, WSWAVE, TEMPXNLEV, CD, UFRIC, Z0M)
    DO IJ = 1, N
      IF (WSWAVE(IJ) < WSPMIN) BR(IJ) = IOR(BR(IJ), BR_WSPMIN)
      IF (Z0M(IJ) == 0.000001_JWRB) BR(IJ) = IOR(BR(IJ), BR_Z0MIN)
    ENDDO
    TAUW(:) = 0.1_JWRB * UFRIC(:)**2
    TAUWDIR(:) = WDWAVE(:)
    IF (HASCD /= 0) THEN
      DO IJ = 1, N
        IF (CDIN(MAPIN(IJ)) /= ZMISS .AND. CDIN(MAPIN(IJ)) > 0.0_JWRB) THEN
          CD(IJ) = CDIN(MAPIN(IJ))
          BR(IJ) = IOR(BR(IJ), BR_CD)
        ENDIF
      ENDDO
      ! buildstress.F90:279-313, restated around the reference's CHNKMIN
      IF (LLCAP /= 0) THEN
        DO IJ = 1, N
          ALPHAOG(IJ) = CHNKMIN(WSWAVE(IJ))*GM1
        ENDDO
      ELSE
        ALPHAOG(:) = ALPHA*GM1
      ENDIF
      DO IJ = 1, N
        UFRIC(IJ) = CD(IJ) * MAX(WSWAVE(IJ)**2, EPSU10**2)
        IF (UFRIC(IJ) < EPSUS) BR(IJ) = IOR(BR(IJ), BR_EPSUS)
        UFRIC(IJ) = MAX(UFRIC(IJ), EPSUS)
        USTAR = SQRT(UFRIC(IJ))
        CDSQRTINV = MIN(1._JWRB/SQRT(CD(IJ)), 50.0_JWRB)
        Z0TOT = TEMPXNLEV*EXP(-XKAPPA*CDSQRTINV)
        ZA = Z0TOT - RNUM/USTAR
        ZB = ALPHAOG(IJ)*UFRIC(IJ)
        IF (ZA < ZB) BR(IJ) = IOR(BR(IJ), BR_FLOOR_Z0M)
        Z0M(IJ) = MAX(Z0TOT - RNUM/USTAR, ALPHAOG(IJ)*UFRIC(IJ))
        CHARNOCKOG = Z0M(IJ)/UFRIC(IJ)
        CHARNOCKOG = MAX(CHARNOCKOG, ALPHAOG(IJ))
        ! clipped, or the rounding of (ALPHAOG UFRIC)/UFRIC against ALPHAOG (tests/restart_ref.py says why the two are one branch)
        IF (UFRIC(IJ)*(1._JWRB-(ALPHAOG(IJ)/CHARNOCKOG)**2) <= 4._JWRB*EPSILON(1._JWRB)*UFRIC(IJ)) BR(IJ) = IOR(BR(IJ), BR_TAUW0)
        TAUW(IJ) = MAX(UFRIC(IJ)*(1._JWRB-(ALPHAOG(IJ)/CHARNOCKOG)**2), 0._JWRB)
        TAUWDIR(IJ) = WDWAVE(IJ)
        CHRNCK(IJ) = G * CHARNOCKOG
        UFRIC(IJ) = USTAR
      ENDDO
    ENDIF
    ! getstress.F90:294-303
    IF (NSE /= 0) THEN
      CHRNCK(:) = PRCHAR
      TAUW(:) = 0.0_JWRB
    ENDIF
    FFO(JWSWAVE,:) = WSWAVE
    FFO(JUFRIC,:) = UFRIC
    FFO(JTAUW,:) = TAUW
    FFO(JTAUWDIR,:) = TAUWDIR
    FFO(JZ0M,:) = Z0M
    FFO(JZ0B,:) = Z0B
    FFO(JCHRNCK,:) = CHRNCK
    WRITE(11) REAL(FFO, 8), REAL(CD, 8), REAL(BR, 8)
  ENDDO

  ! ---- the restart files
  READ(10) FL8
  DO M = 1, NFRE
    DO K = 1, NANG
      DO IJ = 1, N
        FL(IJ,K,M) = REAL(FL8(M,K,IJ), JWRB)
      ENDDO
    ENDDO
  ENDDO
  READ(10) FF8
  FFR = REAL(FF8, JWRB)
  READ(10) V8
  UCUR = REAL(V8, JWRB)
  READ(10) V8
  VCUR = REAL(V8, JWRB)
  READ(10) CDTPRO, CDATEWO, CDAWIFL, CDATEFL
  ALLOCATE(IJ2NEWIJ(N))
  IJ2NEWIJ = PERM
  ! savstress.F90:112-127, restated
  RFIELD(:,1)  = FFR(JWSWAVE,:)
  RFIELD(:,2)  = FFR(JWDWAVE,:)
  RFIELD(:,3)  = FFR(JUFRIC,:)
  RFIELD(:,4)  = FFR(JTAUW,:)
  RFIELD(:,5)  = FFR(JTAUWDIR,:)
  RFIELD(:,6)  = FFR(JZ0M,:)
  RFIELD(:,7)  = FFR(JZ0B,:)
  RFIELD(:,8)  = FFR(JCHRNCK,:)
  RFIELD(:,9)  = FFR(JAIRD,:)
  RFIELD(:,10) = FFR(JWSTAR,:)
  RFIELD(:,11) = FFR(JCICOVER,:)
  RFIELD(:,12) = FFR(JCITHICK,:)
  RFIELD(:,13) = FFR(JUSTRA,:)
  RFIELD(:,14) = FFR(JVSTRA,:)
  RFIELD(:,15) = UCUR
  RFIELD(:,16) = VCUR
  DO IPASS = 1, 2
    IF (IPASS == 1) THEN      ! writefl.F90:113, writestress.F90:101
      LL1D = .TRUE.
      NPROC = 1
    ELSE                      ! writefl.F90:117, writestress.F90:105: a global file of a 2-D decomposition
      LL1D = .FALSE.
      NPROC = 2
    ENDIF
    FILENAME = TRIM(DIR)//MERGE('/BLS_ll1d ', '/BLS_relab', IPASS == 1)
    IUNIT = 0
    CALL WRITEFL(FL, 1, N, 1, NANG, 1, NFRE, FILENAME, IUNIT, .TRUE., .FALSE.)
    FILENAME = TRIM(DIR)//MERGE('/LAW_ll1d ', '/LAW_relab', IPASS == 1)
    CALL WRITESTRESS(1, N, NREAL, RFIELD, FILENAME, .FALSE.)
    CDTPRO = ' '
    RBACK = 0.0_JWRB
    CALL READSTRESS(1, N, NREAL, RBACK, FILENAME, .FALSE.)
    WRITE(11) REAL(RBACK, 8)
  ENDDO
  ! ---- EMAXDPT: initdpthflds.F90:61-73, restated (the routine is bound to the chunks of the model's types)
  READ(10) ND
  ALLOCATE(D8(ND), DEPTH(ND), EMAXDPT(ND))
  READ(10) D8
  DEPTH = REAL(D8, JWRB)
  READ(10) ZREF8
  GAM_B_J = REAL(ZREF8, JWRB)
  DO IJ = 1, ND
    IF (DEPTH(IJ) < 4.0_JWRB) THEN
      GAM=GAM_B_J*DEPTH(IJ)/4.0_JWRB
    ELSE
      GAM=GAM_B_J
    ENDIF
    EMAXDPT(IJ) = 0.0625_JWRB*(GAM*DEPTH(IJ))**2
  ENDDO
  WRITE(11) REAL(EMAXDPT, 8)
  CLOSE(10)
  CLOSE(11)
END PROGRAM RESTART_DRIVER

! the reference's IWAM_GET_UNIT without CONVERT='BIG_ENDIAN' and without its messages: a free unit, the file opened unformatted and sequential
FUNCTION IWAM_GET_UNIT (KUSO, CDNAME, CDACCESS, CDFORM, KRECL, CDACTION)
  USE PARKIND_WAVE, ONLY : JWIM
  IMPLICIT NONE
  INTEGER(KIND=JWIM) :: IWAM_GET_UNIT
  INTEGER(KIND=JWIM), INTENT(IN) :: KUSO
  CHARACTER(LEN=*), INTENT(IN) :: CDNAME, CDACTION
  CHARACTER(LEN=1), INTENT(IN) :: CDACCESS, CDFORM
  INTEGER(KIND=JWIM), INTENT(IN) :: KRECL
  INTEGER(KIND=JWIM) :: JUME
  LOGICAL :: LLUSED
  IF (CDFORM /= 'u') ERROR STOP 9
  DO JUME = 140, 300
    INQUIRE(UNIT=JUME, OPENED=LLUSED)
    IF (.NOT. LLUSED) EXIT
  ENDDO
  IF (CDACCESS == 'a') THEN
    OPEN(UNIT=JUME, FILE=CDNAME, FORM='UNFORMATTED', ACCESS='SEQUENTIAL', POSITION='APPEND', ACTION=CDACTION)
  ELSEIF (CDACCESS == 'w') THEN
    OPEN(UNIT=JUME, FILE=CDNAME, FORM='UNFORMATTED', ACCESS='SEQUENTIAL', STATUS='REPLACE', ACTION=CDACTION)
  ELSE
    OPEN(UNIT=JUME, FILE=CDNAME, FORM='UNFORMATTED', ACCESS='SEQUENTIAL', STATUS='OLD', ACTION=CDACTION)
  ENDIF
  IWAM_GET_UNIT = JUME
END FUNCTION IWAM_GET_UNIT
